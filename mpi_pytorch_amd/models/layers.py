"""NHWC building blocks with torchvision-compatible parameter names and state_dict layout.

Internally conv weights are stored ``[K, R, S, C]`` ("KRSC", the layout the implicit-GEMM
MFMA kernels read with 16-byte vector loads along C) and activations are NHWC.  The
state_dict converts to/from torchvision's OIHW at save/load time, so checkpoints keep the
reference contract (``main.py:163-168``: ``model.state_dict()`` of a torchvision model;
loaded by ``evaluation_pipeline.py:142-144`` / ``helpers.py:13``).

``FusedSequential`` keeps torchvision's ``nn.Sequential`` indices (``features.0``,
``features.1`` ...) but executes Conv->BN->ReLU and Conv->ReLU runs as single fused ops.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import functional as Fn


def _pair(v) -> Tuple[int, int]:
    if isinstance(v, (tuple, list)):
        return int(v[0]), int(v[1])
    return int(v), int(v)


def _pad_rows(n: int) -> int:
    """Stored output width of a padded classifier (Linear / head conv): a multiple of 32."""
    return n if n % 32 == 0 else (n + 31) // 32 * 32


def _krsc_to_oihw(t):
    return t.permute(0, 3, 1, 2)


def _oihw_to_krsc(t):
    return t.permute(0, 2, 3, 1)


_PAIR_STEM = os.environ.get("MPA_PAIR_STEM", "1") == "1"


class Conv2d(nn.Module):
    """Conv2d with KRSC weight storage. ``state_dict`` exposes OIHW like ``nn.Conv2d``.

    Image-input stems (``in_channels < 8``) store their weight with the channel dim
    zero-padded to 8 (``cin_store``): the input images are produced with 8 channels by the
    preprocess kernel, so the stem conv takes the 16-byte vector gather path; the zero
    channels contribute exactly nothing and receive exactly zero gradient.  The padding is
    invisible in state_dict / optimizer state (sliced off on export, re-added on import).

    **Pixel-pair stems** (image input, horizontal stride 2 - the 7x7/s2 stems of ResNet,
    DenseNet and SqueezeNet, Inception's 3x3/s2): the image is stored with 4 channels
    (RGB + 0) on a zero-bordered canvas (``input_spec``, written directly by the preprocess
    kernel), so two horizontally adjacent pixels are one 16-B, 8-"channel" vector.  A
    stride-2 conv with an S-wide kernel over 4-channel pixels is then exactly a stride-1
    conv with a ceil(S/2)-wide kernel over 8-channel pixel pairs, padding 0: weight
    ``[K][R][S][3]`` is stored as ``[K][R][ceil(S/2)][2 x 4]`` (zero for the 4th channel
    and, for odd S, the column past the kernel).  Against the plain 8-channel layout this
    halves the stem's MFMA work (K = R x 32 instead of R x 2 x 32 for 7x7), its wgrad
    columns (224 vs 392) and the image bytes.  The column past an odd kernel would get a
    nonzero gradient (its input pixels are real), so ``fix_grad`` zeroes it after wgrad;
    the 4th channel's gradient is exactly zero (its input is).
    """

    def __init__(self, in_channels: int, out_channels: int, kernel_size, stride=1, padding=0,
                 bias: bool = True, pad_out: bool = False, groups: int = 1):
        super().__init__()
        kh0, kw0 = _pair(kernel_size)
        # grouped: the geometries the gconv kernels take (conv_group.hip): 3x3, padding 1, one
        # stride in {1, 2}, in == out channels a multiple of 16, 4 / 8 / 16 / 32 per group
        self.grouped = (groups != 1 and groups != in_channels and in_channels == out_channels
                        and in_channels % 16 == 0 and in_channels % groups == 0
                        and in_channels // groups in (4, 8, 16, 32) and (kh0, kw0) == (3, 3)
                        and _pair(padding) == (1, 1) and _pair(stride) in ((1, 1), (2, 2)))
        if groups != 1 and not self.grouped and not (groups == in_channels == out_channels):
            raise ValueError("Conv2d: groups must be 1, in_channels == out_channels (depthwise) "
                             "or a grouped 3x3 (padding 1, stride 1 or 2, equal channels % 16 == "
                             "0, 4 / 8 / 16 / 32 per group), got groups={} for {} -> {} channels, "
                             "kernel {}".format(groups, in_channels, out_channels, (kh0, kw0)))
        self.groups = groups
        # depthwise: weight stored [C, R, S, 1] (OIHW [C, 1, R, S]), run by the dwconv kernels
        # (Fn.dwconv); no channel padding, no pixel pairs, no transposed copy (the kernels
        # transpose their channel chunk of the stored weight while staging it).  grouped: weight
        # stored [C, 3, 3, Cg] (OIHW [C, Cg, 3, 3]), run by the gconv kernels (Fn.gconv), which
        # expand and transpose it while they build their MFMA fragments
        self.depthwise = groups != 1 and not self.grouped
        self.cin_w = in_channels // groups  # the weight's input-channel extent
        self.in_channels = in_channels
        self.pair = (_PAIR_STEM and in_channels <= 4 and _pair(stride)[1] == 2 and kw0 >= 2)
        self.cin_store = 8 if in_channels < 8 else in_channels
        if self.depthwise or self.grouped:
            self.pair, self.cin_store = False, self.cin_w
        self.out_channels = out_channels
        # pad_out: store the output channels rounded up to a multiple of 32 (zero filters) -
        # for classifier convs (SqueezeNet's 512 -> 64,500 1x1 head) so their dgrad / wgrad
        # stay on the 16-B LDS-DMA paths; the model slices the logits back
        self.cout_store = _pad_rows(out_channels) if pad_out else out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = _pair(stride)
        self.padding = _pair(padding)
        kh, kw = self.kernel_size
        self.sp = (kw + 1) // 2  # pixel-pair kernel width
        # geometry of the conv the kernels actually run: (sh, sw, ph, pw)
        if self.pair:
            self.kgeom = (self.stride[0], 1, 0, 0)
        else:
            self.kgeom = (self.stride[0], self.stride[1], self.padding[0], self.padding[1])
        w = torch.empty(out_channels, self.cin_w, kh, kw)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        self.weight = nn.Parameter(self._imp(w).contiguous())
        self.weight._mpa_export = self._exp
        self.weight._mpa_import = self._imp
        # (K, R*S, C) of the stored KRSC weight: the arena keeps a [C][R*S][K] copy for dgrad
        ks = self.sp if self.pair else kw
        if not self.depthwise and not self.grouped:
            self.weight._mpa_tlayout = (self.cout_store, kh * ks, self.cin_store)
        if bias:
            fan_in = self.cin_w * kh * kw
            bound = 1 / math.sqrt(fan_in)
            b = torch.empty(out_channels).uniform_(-bound, bound)
            self.bias = nn.Parameter(self._imp_bias(b))
            if self.cout_store != out_channels:
                self.bias._mpa_export = self._exp_bias
                self.bias._mpa_import = self._imp_bias
        else:
            self.register_parameter("bias", None)

    def _exp(self, t):  # internal KRSC (maybe channel padded / pixel pairs) -> OIHW
        if self.pair:  # [K][R][Sp][2 x 4] -> [K][R][S][3]
            kh, kw = self.kernel_size
            t = t.reshape(t.shape[0], kh, 2 * self.sp, 4)[:, :, :kw, :self.in_channels]
        elif self.cin_store != self.cin_w:
            t = t[..., :self.in_channels]
        if self.cout_store != self.out_channels:
            t = t[:self.out_channels]
        return _krsc_to_oihw(t)

    def _imp(self, t):  # OIHW -> internal KRSC
        t = _oihw_to_krsc(t)
        if self.pair:
            kh, kw = self.kernel_size
            t = F.pad(t, (0, 4 - self.in_channels, 0, 2 * self.sp - kw))
            t = t.reshape(t.shape[0], kh, self.sp, 8)
        elif self.cin_store != self.cin_w:
            t = F.pad(t, (0, self.cin_store - self.in_channels))
        if t.shape[0] < self.cout_store:
            t = F.pad(t, (0, 0, 0, 0, 0, 0, 0, self.cout_store - t.shape[0]))
        return t

    def _exp_bias(self, t):
        return t[:self.out_channels]

    def _imp_bias(self, t):
        return F.pad(t, (0, self.cout_store - t.shape[0])) if t.shape[0] < self.cout_store else t

    # init helpers operate in OIHW space so the distributions match torchvision
    def init_(self, fn) -> "Conv2d":
        with torch.no_grad():
            w = torch.empty(self.out_channels, self.cin_w, *self.kernel_size)
            fn(w)
            self.weight.copy_(self._imp(w))
        return self

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        k = prefix + "weight"
        if k in destination:
            w = destination[k]
            destination[k] = self._exp(w) if keep_vars else self._exp(w).contiguous()
        k = prefix + "bias"
        if k in destination and destination[k] is not None and self.cout_store != self.out_channels:
            b = self._exp_bias(destination[k])
            destination[k] = b if keep_vars else b.contiguous()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys,
                              unexpected_keys, error_msgs):
        k = prefix + "weight"
        if k in state_dict:
            w = state_dict[k]
            if tuple(w.shape) == (self.out_channels, self.cin_w, *self.kernel_size):
                state_dict[k] = self._imp(w)
        k = prefix + "bias"
        if k in state_dict and tuple(state_dict[k].shape) == (self.out_channels,):
            state_dict[k] = self._imp_bias(state_dict[k])
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys,
                                      unexpected_keys, error_msgs)

    def forward(self, x, relu: bool = False):
        if self.depthwise:
            y = Fn.dwconv(x, self)
            return ReLU()(y) if relu else y
        if self.grouped:
            y = Fn.gconv(x, self)
            return ReLU()(y) if relu else y
        return Fn.conv_act(x, self, relu=relu)

    def input_spec(self, hw) -> dict:
        """Layout the data pipeline should produce for an ``hw`` image fed to this conv:
        ``cpad`` channels on a zero canvas ``pad`` = (top, bottom, left, right)."""
        if not self.pair:
            return {"cpad": self.cin_store, "pad": None}
        H, W = hw
        (kh, kw), (ph, pw) = self.kernel_size, self.padding
        Q = (W + 2 * pw - kw) // 2 + 1
        right = 2 * (Q - 1 + self.sp) - W - pw
        return {"cpad": 4, "pad": (ph, ph, pw, right)}

    def fit_input(self, x):
        """Bring an image input into the stored layout.  Plain convs: zero-pad the channel
        dim to the stored width (no-op normally).  Pixel-pair stems: a 4-channel input is
        taken to be the pre-padded canvas of ``input_spec`` (what the data pipeline
        produces); 3/8-channel images are converted here.  Returns the [N][Hp][Wp/2][8]
        pixel-pair view."""
        c = x.shape[-1]
        if self.pair:
            if c != 4:
                N, H, W = x.shape[:3]
                t, b, l, r = self.input_spec((H, W))["pad"]
                if r < 0:
                    raise ValueError("pixel-pair stem: image width %d too small" % W)
                x = F.pad(x[..., :3], (0, 1, l, r, t, b))
            N, Hp, Wp = x.shape[:3]
            if Wp % 2:
                raise ValueError("pixel-pair stem: canvas width %d is odd" % Wp)
            return x.contiguous().view(N, Hp, Wp // 2, 8)
        if c < self.cin_store:
            x = F.pad(x, (0, self.cin_store - c))
        return x

    def fix_grad(self, g) -> None:
        """Pixel-pair stem with an odd kernel width: the stored column past the kernel
        (second pixel of the last pair) must keep exactly zero weight."""
        kw = self.kernel_size[1]
        if self.pair and kw % 2 and g is not None:
            # g as [K * kh][sp * 8]: the last pair's second pixel = columns (sp-1)*8+4 .. sp*8
            Fn.K(g).zero_cols_f32(g, self.sp * 8, (self.sp - 1) * 8 + 4, 4)

    def extra_repr(self):
        return "{}, {}, kernel_size={}, stride={}, padding={}, bias={}{}".format(
            self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding,
            self.bias is not None, ", groups=%d" % self.groups if self.groups != 1 else "")


class BatchNorm2d(nn.Module):
    """BatchNorm over the channel (last, NHWC) dim; same names/buffers as nn.BatchNorm2d."""

    def __init__(self, num_features: int, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        # host shadow of num_batches_tracked (the device buffer is bumped inside the BN
        # kernel): momentum=None's cumulative average needs the count without a device sync
        self._batches_host = 0

    def momentum_value(self) -> float:
        """Momentum for this training step (nn.BatchNorm2d semantics, incl. None = cumulative
        moving average 1 / num_batches_tracked), advancing the host batch count."""
        self._batches_host += 1
        if self.momentum is None:
            return 1.0 / self._batches_host
        return float(self.momentum)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        key = prefix + "num_batches_tracked"
        if key in state_dict:
            self._batches_host = int(state_dict[key])

    def forward(self, x, relu: bool = False, stats=None):
        return Fn.bn_act(x, self, relu=relu, stats=stats)

    def extra_repr(self):
        return "{}, eps={}, momentum={}".format(self.num_features, self.eps, self.momentum)


class Linear(nn.Module):
    """Linear layer.  ``in_chw=(C,H,W)`` marks a layer fed by an NHWC flatten: its input
    columns are stored in (h,w,c) order internally and exported in torchvision's
    NCHW-flatten (c,h,w) order.

    The output dim is stored rounded up to a multiple of 32 (``out_store``) with zero
    weight rows and bias entries: a 64,500-class head becomes 64,512 rows, so its forward,
    dgrad, wgrad and bias-gradient all run on the 16-B-granular LDS-DMA GEMM paths
    instead of scalar/8-byte fallbacks.  ``forward`` returns the first ``out_features``
    columns (a view); the padding is invisible in state_dict and optimizer state, and the
    padded rows never receive gradient (the cross-entropy backward writes zeros there).
    """

    def __init__(self, in_features: int, out_features: int, bias: bool = True,
                 in_chw: Optional[Tuple[int, int, int]] = None):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.out_store = _pad_rows(out_features)
        self.in_chw = in_chw
        w = torch.empty(out_features, in_features)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        self.weight = nn.Parameter(self._imp(w).contiguous())
        if in_chw is not None or self.out_store != out_features:
            self.weight._mpa_export = self._exp
            self.weight._mpa_import = self._imp
        # [in][out] copy for dgrad - except for the wide classifier heads (64,500 classes):
        # their dgrad (M = batch, N = in, K = 64,512, split-K) reads the forward weight with
        # transposing LDS loads as fast or faster (tools/bench_head.py: 61.9 vs 65.7 us), and
        # skipping the copy saves transposing 33 M weights (~24 us) after every update
        if out_features < 16384:
            self.weight._mpa_tlayout = (self.out_store, 1, in_features)
        if bias:
            bound = 1 / math.sqrt(in_features)
            b = torch.empty(out_features).uniform_(-bound, bound)
            self.bias = nn.Parameter(self._imp_bias(b))
            if self.out_store != out_features:
                self.bias._mpa_export = self._exp_bias
                self.bias._mpa_import = self._imp_bias
        else:
            self.register_parameter("bias", None)

    def _exp(self, t):  # internal (o_store, h*w*c) -> torchvision (o, c*h*w)
        t = t[:self.out_features]
        if self.in_chw is None:
            return t
        C, H, W = self.in_chw
        return t.reshape(t.shape[0], H, W, C).permute(0, 3, 1, 2).reshape(t.shape[0], C * H * W)

    def _imp(self, t):
        if self.in_chw is not None:
            C, H, W = self.in_chw
            t = t.reshape(t.shape[0], C, H, W).permute(0, 2, 3, 1).reshape(t.shape[0], H * W * C)
        if t.shape[0] < self.out_store:
            t = F.pad(t, (0, 0, 0, self.out_store - t.shape[0]))
        return t

    def _exp_bias(self, t):
        return t[:self.out_features]

    def _imp_bias(self, t):
        return F.pad(t, (0, self.out_store - t.shape[0])) if t.shape[0] < self.out_store else t

    def init_(self, fn) -> "Linear":
        with torch.no_grad():
            w = torch.empty(self.out_features, self.in_features)
            fn(w)
            self.weight.copy_(self._imp(w))
        return self

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        k = prefix + "weight"
        if k in destination:
            w = self._exp(destination[k])
            destination[k] = w if keep_vars else w.contiguous()
        k = prefix + "bias"
        if k in destination and destination[k] is not None:
            b = self._exp_bias(destination[k])
            destination[k] = b if keep_vars else b.contiguous()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys,
                              unexpected_keys, error_msgs):
        k = prefix + "weight"
        if k in state_dict and tuple(state_dict[k].shape) == (self.out_features, self.in_features):
            state_dict[k] = self._imp(state_dict[k])
        k = prefix + "bias"
        if k in state_dict and tuple(state_dict[k].shape) == (self.out_features,):
            state_dict[k] = self._imp_bias(state_dict[k])
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys,
                                      unexpected_keys, error_msgs)

    def forward(self, x, relu: bool = False):
        return Fn.linear_act(x, self, relu=relu)

    def extra_repr(self):
        return "in_features={}, out_features={}, bias={}".format(
            self.in_features, self.out_features, self.bias is not None)


class ReLU(nn.Module):
    def __init__(self, inplace: bool = False):
        super().__init__()

    def forward(self, x):
        # only reached when not fused into a producer; keep it a kernel op
        return Fn.K(x).relu_fwd(x) if not x.requires_grad else _relu_autograd(x)


def _relu_autograd(x):
    return _ReLUFn.apply(x)


class _ReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = Fn.K(x).relu_fwd(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return Fn.K(dy).act_bwd(dy.contiguous(), y, Fn._empty(dy))


class Hardswish(nn.Module):
    """x * relu6(x + 3) / 6.  Behind a BatchNorm the models fuse it into ``Fn.bn_act_gate``; this
    module is the stand-alone form (MobileNetV3's classifier)."""

    def __init__(self, inplace: bool = False):
        super().__init__()

    def forward(self, x):
        return Fn.hardswish(x)


class LayerNorm(nn.Module):
    """LayerNorm over the last (channel) axis of an NHWC or [rows, C] activation: torchvision's
    ``LayerNorm2d`` (which normalises NCHW's channel axis) and ``nn.LayerNorm(C)`` alike, with
    their parameter names."""

    def __init__(self, normalized_shape: int, eps: float = 1e-6):
        super().__init__()
        self.normalized_shape = (int(normalized_shape),)
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))

    def forward(self, x):
        return Fn.layer_norm(x, self)

    def extra_repr(self):
        return "{}, eps={}".format(self.normalized_shape, self.eps)


class GELU(nn.Module):
    """Exact (erf) GELU.  Behind a Linear the models fuse it into ``Fn.linear_gelu``."""

    def forward(self, x):
        return Fn.gelu(x)


class _InProj:
    """The packed q/k/v projection of a MultiheadAttention as the layer ``Fn.linear_act`` reads."""

    def __init__(self, mha):
        self._mha = mha
        self.out_features = 3 * mha.embed_dim

    @property
    def weight(self):
        return self._mha.in_proj_weight

    @property
    def bias(self):
        return self._mha.in_proj_bias


class MultiheadAttention(nn.Module):
    """Self-attention with ``torch.nn.MultiheadAttention``'s parameter names and q/k/v row
    order: ``in_proj_weight`` [3 D, D], ``in_proj_bias`` [3 D], ``out_proj``.  Head dim 64.  The
    in-projection's rows [B S, 3 D] are the attention kernel's packed input as they are, and its
    output [B, S, D] is the out-projection's rows: no permute or split in between."""

    def __init__(self, embed_dim: int, num_heads: int):
        super().__init__()
        if embed_dim != 64 * num_heads:
            raise ValueError("MultiheadAttention: head dim must be 64 (embed_dim = 64 * num_heads)")
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_weight._mpa_tlayout = (3 * embed_dim, 1, embed_dim)
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)
        self._in = _InProj(self)

    def forward(self, rows, B: int, S: int):
        """rows [B S, D] -> [B S, D]"""
        D = self.embed_dim
        qkv = Fn.linear_act(rows, self._in).reshape(B, S, 3 * D)
        o = Fn.attention(qkv, self.num_heads)
        return Fn.linear_act(o.reshape(B * S, D), self.out_proj)

    def extra_repr(self):
        return "embed_dim={}, num_heads={}".format(self.embed_dim, self.num_heads)


class ShiftedWindowAttention(nn.Module):
    """Swin's window attention with torchvision's names: ``qkv``, ``proj``,
    ``relative_position_bias_table`` and the ``relative_position_index`` buffer.  Head dim 32.
    The in-projection's rows [B Hf Wf, 3 D] are the kernel's input in natural token order and its
    output rows are the out-projection's input: roll, window partition and reverse are the
    kernel's address arithmetic, the bias gather and the shift mask its register arithmetic.

    The table is stored flat, head-major [H (2 ws - 1)^2] (1-D: left out of weight decay and
    trust ratio like ``pos_embedding``), and is [(2 ws - 1)^2, H] in the state_dict.  The int64
    index buffer exists for state_dict parity only: no kernel reads it."""

    def __init__(self, dim: int, window: int, shift: int, num_heads: int):
        super().__init__()
        if dim != 32 * num_heads:
            raise ValueError("ShiftedWindowAttention: head dim must be 32 (dim = 32 * num_heads)")
        if window * window > 64 or not 0 <= shift < window:
            raise ValueError("ShiftedWindowAttention: window^2 <= 64 and 0 <= shift < window")
        self.dim, self.window, self.shift, self.num_heads = dim, window, shift, num_heads
        self.qkv = Linear(dim, 3 * dim)
        self.proj = Linear(dim, dim)
        nb = (2 * window - 1) ** 2
        self.relative_position_bias_table = nn.Parameter(
            nn.init.trunc_normal_(torch.empty(num_heads * nb), std=0.02))
        self.relative_position_bias_table._mpa_export = self._exp_table
        self.relative_position_bias_table._mpa_import = self._imp_table
        self.register_buffer("relative_position_index", Fn.ref.swin_relative_index(window).flatten())

    def _exp_table(self, t):
        return t.reshape(self.num_heads, -1).t()

    @staticmethod
    def _imp_table(t):
        return t.t().reshape(-1)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        k = prefix + "relative_position_bias_table"
        if k in destination:
            t = self._exp_table(destination[k])
            destination[k] = t if keep_vars else t.contiguous()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = prefix + "relative_position_bias_table"
        if k in state_dict and state_dict[k].dim() == 2:
            state_dict[k] = self._imp_table(state_dict[k])
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, rows, Hf: int, Wf: int):
        """rows [B Hf Wf, D] -> [B Hf Wf, D]"""
        shift = 0 if min(Hf, Wf) <= self.window else self.shift  # one window: nothing to shift
        qkv = Fn.linear_act(rows, self.qkv)
        if not qkv.is_contiguous():
            qkv = qkv.contiguous()
        o = Fn.window_attention(qkv, self.relative_position_bias_table, self.num_heads, Hf, Wf,
                                self.window, shift)
        return Fn.linear_act(o, self.proj)

    def extra_repr(self):
        return "dim={}, window={}, shift={}, num_heads={}".format(self.dim, self.window, self.shift,
                                                                  self.num_heads)


class NeighborhoodAttention(nn.Module):
    """NAT's attention with the official names: ``qkv``, ``rpb`` [heads, 13, 13] and ``proj``.
    Head dim 32, neighbourhood 7.  The in-projection's rows [B Hf Wf, 3 D] are the kernel's input
    in natural token order and its output rows are the out-projection's input: the 49 keys of a
    pixel are the kernel's address arithmetic, the bias gather its register arithmetic."""

    def __init__(self, dim: int, num_heads: int):
        super().__init__()
        if dim != 32 * num_heads:
            raise ValueError("NeighborhoodAttention: head dim must be 32 (dim = 32 * num_heads)")
        self.dim, self.num_heads = dim, num_heads
        self.qkv = Linear(dim, 3 * dim)
        self.rpb = nn.Parameter(nn.init.trunc_normal_(torch.empty(num_heads, 13, 13), std=0.02))
        self.proj = Linear(dim, dim)

    def forward(self, rows, Hf: int, Wf: int):
        """rows [B Hf Wf, D] -> [B Hf Wf, D]"""
        qkv = Fn.linear_act(rows, self.qkv)
        if not qkv.is_contiguous():
            qkv = qkv.contiguous()
        return Fn.linear_act(Fn.neighborhood_attention(qkv, self.rpb, self.num_heads, Hf, Wf), self.proj)

    def extra_repr(self):
        return "dim={}, num_heads={}".format(self.dim, self.num_heads)


class SpatialReductionAttention(nn.Module):
    """PVT v2's attention with the official names: ``q``, ``kv``, ``proj`` and, where ``sr_ratio``
    > 1, the reduction ``sr`` (a conv with kernel = stride = sr_ratio, run as ``Fn.patch_rows`` and
    the rows GEMM: the strided-conv dgrad serves at most 16 stride phases, stride 8 has 64) and its
    LayerNorm ``norm``.  The map must be a multiple of sr_ratio (the official conv drops the rest).
    Head dim 64.  Every token of the map is a query; keys and values come from the reduced map,
    at most 64 tokens (``Fn.cross_attention``).  The q rows [B Hf Wf, D] and the kv rows [B Sk,
    2 D] are the kernel's inputs as they are, and its output the out-projection's rows."""

    MAX_KEYS = 64

    def __init__(self, dim: int, num_heads: int, sr_ratio: int = 1):
        super().__init__()
        if dim != 64 * num_heads:
            raise ValueError("SpatialReductionAttention: head dim must be 64 (dim = 64 * num_heads)")
        self.dim, self.num_heads, self.sr_ratio = dim, num_heads, sr_ratio
        self.q = Linear(dim, dim)
        self.kv = Linear(dim, 2 * dim)
        self.proj = Linear(dim, dim)
        if sr_ratio > 1:
            # kernel = stride: ``patchify`` and the rows GEMM, weight OIHW in the state_dict
            self.sr = PatchEmbed(dim, dim, sr_ratio, cin_store=dim)
            self.norm = LayerNorm(dim, eps=1e-5)

    def forward(self, x):
        """x [B, Hf, Wf, D] -> [B, Hf, Wf, D]"""
        B, Hf, Wf, D = x.shape
        r = self.sr_ratio
        if Hf % r or Wf % r:
            raise ValueError("SpatialReductionAttention: the map must be a multiple of sr_ratio")
        Sk = (Hf // r) * (Wf // r)
        if not 1 <= Sk <= self.MAX_KEYS:
            raise ValueError("SpatialReductionAttention: the reduced map holds {} tokens; the "
                             "attention kernel serves 1 to {} keys".format(Sk, self.MAX_KEYS))
        xq, xk = Fn.fan_out(x, 2)
        q = Fn.linear_act(xq.reshape(B * Hf * Wf, D), self.q)
        if r > 1:
            xk = self.norm(Fn.linear_act(Fn.patch_rows(xk, r), self.sr))
        kv = Fn.linear_act(xk.reshape(B * Sk, D), self.kv)
        o = Fn.cross_attention(q.reshape(B, Hf * Wf, D), kv.reshape(B, Sk, 2 * D), self.num_heads)
        return Fn.linear_act(o.reshape(B * Hf * Wf, D), self.proj).reshape(B, Hf, Wf, D)

    def extra_repr(self):
        return "dim={}, num_heads={}, sr_ratio={}".format(self.dim, self.num_heads, self.sr_ratio)


class _MlpLayer(nn.Module):
    """``weight`` [out, in] and ``bias`` of one layer of the position-bias MLP, stored as they
    are (fp32, no pad rows): ``Fn.cpb_bias`` reads both layers in one kernel."""

    def __init__(self, in_features: int, out_features: int, bias: bool):
        super().__init__()
        self.weight = nn.Parameter(nn.init.trunc_normal_(torch.empty(out_features, in_features), std=0.02))
        self.bias = nn.Parameter(torch.zeros(out_features)) if bias else None


class ShiftedWindowAttentionV2(nn.Module):
    """Swin V2's window attention with torchvision's names: ``qkv``, ``proj``, ``logit_scale``,
    ``cpb_mlp.0.weight / bias``, ``cpb_mlp.2.weight`` and the ``relative_coords_table`` and
    ``relative_position_index`` buffers.  Head dim 32.  Scores are cosines times the clamped
    temperature exp(min(logit_scale, ln 100)) plus 16 sigmoid(cpb_mlp(log-spaced offsets)):
    ``Fn.cpb_bias`` writes the table in fp32, ``Fn.window_attention_cos`` reads the
    in-projection's rows in natural token order and normalises inside the score tile.

    ``logit_scale`` is stored flat [H] (1-D: left out of weight decay and trust ratio) and is
    [H, 1, 1] in the state_dict.  The k third of the qkv bias is treated as zero, as torchvision
    does in its forward: it is zero at construction and on import, and its gradient is cleared
    in the in-projection's backward, so it stays zero.  The two buffers exist for state_dict
    parity only: no kernel reads them."""

    def __init__(self, dim: int, window: int, shift: int, num_heads: int):
        super().__init__()
        if dim != 32 * num_heads:
            raise ValueError("ShiftedWindowAttentionV2: head dim must be 32 (dim = 32 * num_heads)")
        if window < 2 or window * window > 64 or not 0 <= shift < window:
            raise ValueError("ShiftedWindowAttentionV2: 2 <= window, window^2 <= 64, 0 <= shift < window")
        self.dim, self.window, self.shift, self.num_heads = dim, window, shift, num_heads
        self.qkv = Linear(dim, 3 * dim)
        self.proj = Linear(dim, dim)
        self._zero_k_bias()
        self.logit_scale = nn.Parameter(torch.full((num_heads,), math.log(10.0)))
        self.logit_scale._mpa_export = self._exp_scale
        self.logit_scale._mpa_import = self._imp_scale
        self.cpb_mlp = nn.Sequential(_MlpLayer(2, 512, True), nn.Identity(), _MlpLayer(512, num_heads, False))
        c = torch.arange(-(window - 1), window, dtype=torch.float32)
        t = torch.stack(torch.meshgrid([c, c], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
        t = t / (window - 1) * 8
        self.register_buffer("relative_coords_table", torch.sign(t) * torch.log2(t.abs() + 1.0) / 3.0)
        self.register_buffer("relative_position_index", Fn.ref.swin_relative_index(window).flatten())

    @staticmethod
    def _exp_scale(t):
        return t.reshape(-1, 1, 1)

    @staticmethod
    def _imp_scale(t):
        return t.reshape(-1)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        k = prefix + "logit_scale"
        if k in destination:
            destination[k] = self._exp_scale(destination[k])

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = prefix + "logit_scale"
        if k in state_dict and state_dict[k].dim() == 3:
            state_dict[k] = self._imp_scale(state_dict[k])
        k = prefix + "qkv.bias"
        if k in state_dict:  # (the child module loads it after this hook)
            state_dict[k] = state_dict[k].clone()
            state_dict[k][self.dim:2 * self.dim] = 0
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _zero_k_bias(self):
        with torch.no_grad():
            self.qkv.bias[self.dim:2 * self.dim].zero_()

    def forward(self, rows, Hf: int, Wf: int):
        """rows [B Hf Wf, D] -> [B Hf Wf, D]"""
        shift = 0 if min(Hf, Wf) <= self.window else self.shift  # one window: nothing to shift
        qkv = Fn.linear_act(rows, self.qkv, dead_bias=(self.dim, 2 * self.dim))
        if not qkv.is_contiguous():
            qkv = qkv.contiguous()
        mlp = self.cpb_mlp
        bias = Fn.cpb_bias(mlp[0].weight, mlp[0].bias, mlp[2].weight, self.num_heads, self.window)
        o = Fn.window_attention_cos(qkv, self.logit_scale, bias, self.num_heads, Hf, Wf, self.window, shift)
        return Fn.linear_act(o, self.proj)

    def extra_repr(self):
        return "dim={}, window={}, shift={}, num_heads={}".format(self.dim, self.window, self.shift,
                                                                  self.num_heads)


class PatchEmbed(nn.Module):
    """ViT's patch embedding, a P x P / stride P conv, as patch rows times a [D, P P Cp] matrix
    (``Fn.patch_tokens``).  The state_dict holds torchvision's ``weight`` [D, C, P, P] and
    ``bias``; stored (ky, kx, c) with zero columns for the image's pad channels."""

    def __init__(self, in_channels: int, width: int, patch: int, cin_store: int = 8):
        super().__init__()
        if width % 32:
            raise ValueError("PatchEmbed: width must be a multiple of 32")
        self.in_channels, self.out_features, self.patch, self.cin_store = in_channels, width, patch, cin_store
        fan_in = in_channels * patch * patch
        w = torch.empty(width, in_channels, patch, patch)
        nn.init.trunc_normal_(w, std=math.sqrt(1.0 / fan_in))
        self.weight = nn.Parameter(self._imp(w).contiguous())
        self.weight._mpa_export = self._exp
        self.weight._mpa_import = self._imp
        self.weight._mpa_tlayout = (width, 1, patch * patch * cin_store)
        self.bias = nn.Parameter(torch.zeros(width))

    def _exp(self, t):
        P = self.patch
        t = t.reshape(t.shape[0], P, P, self.cin_store)[..., :self.in_channels]
        return t.permute(0, 3, 1, 2)

    def _imp(self, t):
        t = F.pad(t.permute(0, 2, 3, 1), (0, self.cin_store - self.in_channels))
        return t.reshape(t.shape[0], -1)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        k = prefix + "weight"
        if k in destination:
            w = self._exp(destination[k])
            destination[k] = w if keep_vars else w.contiguous()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = prefix + "weight"
        if k in state_dict and state_dict[k].dim() == 4:
            state_dict[k] = self._imp(state_dict[k])
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def fit_input(self, x):
        c = x.shape[-1]
        if c > self.cin_store:
            raise ValueError("PatchEmbed: %d input channels, %d stored" % (c, self.cin_store))
        return F.pad(x, (0, self.cin_store - c)) if c < self.cin_store else x

    def extra_repr(self):
        return "{}, {}, patch={}".format(self.in_channels, self.out_features, self.patch)


class SqueezeExcitation(nn.Module):
    """torchvision's SqueezeExcitation: ``fc1`` / ``fc2`` are 1x1 convs with bias (OIHW in the
    state_dict), ReLU after the first and hardsigmoid after the second.  It has no forward of
    its own: the gate scales the activation its BatchNorm feeds, so the layer is passed to
    ``Fn.bn_act_gate`` / ``Fn.dwconv_bn_act_gate`` as ``se``."""

    def __init__(self, channels: int, squeeze: int):
        super().__init__()
        self.fc1 = Conv2d(channels, squeeze, 1)
        self.fc2 = Conv2d(squeeze, channels, 1)

    def forward(self, x):
        raise RuntimeError("SqueezeExcitation is applied by Fn.bn_act_gate(z, bn, act, se=layer)")


class MaxPool2d(nn.Module):
    def __init__(self, kernel_size, stride=None, padding=0, ceil_mode=False):
        super().__init__()
        self.kernel_size = _pair(kernel_size)
        self.stride = _pair(stride if stride is not None else kernel_size)
        self.padding = _pair(padding)
        self.ceil_mode = ceil_mode

    def forward(self, x):
        return Fn.max_pool2d(x, self.kernel_size, self.stride, self.padding, self.ceil_mode)


class AvgPool2d(nn.Module):
    def __init__(self, kernel_size, stride=None, padding=0, ceil_mode=False,
                 count_include_pad=True):
        super().__init__()
        self.kernel_size = _pair(kernel_size)
        self.stride = _pair(stride if stride is not None else kernel_size)
        self.padding = _pair(padding)
        self.ceil_mode = ceil_mode
        self.count_include_pad = count_include_pad

    def forward(self, x):
        return Fn.avg_pool2d(x, self.kernel_size, self.stride, self.padding, self.ceil_mode,
                             self.count_include_pad)


class AdaptiveAvgPool2d(nn.Module):
    def __init__(self, output_size):
        super().__init__()
        self.output_size = _pair(output_size)

    def forward(self, x):
        return Fn.adaptive_avg_pool2d(x, self.output_size)


class Dropout(nn.Module):
    def __init__(self, p: float = 0.5, inplace: bool = False):
        super().__init__()
        self.p = p

    def forward(self, x):
        return Fn.dropout(x, self.p, self.training)


class Flatten(nn.Module):
    def forward(self, x):
        return x.reshape(x.shape[0], -1)


# MPA_SEQ_LINK=0: conv -> ReLU -> conv chains of the feature stacks run the separate ReLU
# backward (act_bwd) / BN reduce pass instead of the consumer dgrad's fused reduction
_LINK = os.environ.get("MPA_SEQ_LINK", "1") == "1"


class FusedSequential(nn.Sequential):
    """``nn.Sequential`` with torchvision indices, executed with producer fusion:
    Conv(no bias)->BN[->ReLU] => conv_bn_act; Conv->ReLU => conv_act(relu); Linear->ReLU
    => linear_act(relu)."""

    def groups(self):
        """The fused execution groups: (first index, end index, kind) over the children."""
        mods = list(self._modules.values())
        out, i, n = [], 0, len(mods)
        while i < n:
            m = mods[i]
            nxt = mods[i + 1] if i + 1 < n else None
            nxt2 = mods[i + 2] if i + 2 < n else None
            if isinstance(m, Conv2d) and isinstance(nxt, BatchNorm2d):
                k = 3 if isinstance(nxt2, ReLU) else 2
                out.append((i, i + k, "conv_bn_relu" if k == 3 else "conv_bn"))
            elif isinstance(m, (Conv2d, Linear, BatchNorm2d)) and isinstance(nxt, ReLU):
                k = 2
                out.append((i, i + 2, "relu"))
            else:
                k = 1
                out.append((i, i + 1, "plain"))
            i += k
        return out

    def run_group(self, g, x, link_in=None, link_out=None):
        """Execute fused group ``g`` = (first, end, kind) of :meth:`groups` on ``x``;
        ``link_in`` / ``link_out``: BN-backward hand-offs (Fn.BNLink) with the neighbouring
        conv group (see :meth:`links`)."""
        mods = list(self._modules.values())
        i, _e, kind = g
        if kind.startswith("conv_bn"):
            return Fn.conv_bn_act(x, mods[i], mods[i + 1], relu=kind == "conv_bn_relu",
                                  link_in=link_in, link_out=link_out)
        if kind == "relu":
            if isinstance(mods[i], Conv2d):
                return Fn.conv_act(x, mods[i], relu=True, link_in=link_in, link_out=link_out)
            return mods[i](x, relu=True)
        if link_in is not None and isinstance(mods[i], MaxPool2d):
            m = mods[i]
            return Fn.max_pool2d(x, m.kernel_size, m.stride, m.padding, m.ceil_mode,
                                 link_in=link_in)
        return mods[i](x)

    def links(self, gs):
        """Which consecutive groups hand the backward over: a conv -> (BN ->) ReLU group
        whose output feeds ONLY the next conv group (VGG / AlexNet feature stacks).  The
        consumer's dgrad then applies the producer's ReLU mask and reduces its BN (or
        bias) gradient sums in its epilogue - no reduce / act_bwd pass (Fn.BNLink)."""
        mods = list(self._modules.values())
        out = [False] * len(gs)
        if not (self.training and torch.is_grad_enabled() and _LINK):
            return out
        for k in range(len(gs) - 1):
            (i, _e, kind), (j, _f, kind2) = gs[k], gs[k + 1]
            if (kind in ("relu", "conv_bn_relu") and isinstance(mods[i], Conv2d)
                    and kind2 in ("relu", "conv_bn_relu", "conv_bn")
                    and isinstance(mods[j], Conv2d) and not mods[j].pair):
                out[k] = True
            # conv -> ReLU -> 2x2/s2 max pool (VGG block ends): the pool's backward applies
            # the ReLU mask and reduces the conv's bias gradient (no act_bwd pass)
            m = mods[j]
            if (kind == "relu" and isinstance(mods[i], Conv2d) and kind2 == "plain"
                    and isinstance(m, MaxPool2d) and m.kernel_size == (2, 2)
                    and m.stride == (2, 2) and m.padding == (0, 0)):
                out[k] = True
        return out

    def forward(self, x):
        run = self.run_group
        gs = self.groups()
        lk = self.links(gs)
        link = None
        for k, g in enumerate(gs):
            nxt = Fn.BNLink() if lk[k] else None
            x = run(g, x, link_in=link, link_out=nxt)
            link = nxt
        return x
