"""Swin-T (torchvision ``swin_t``): parameter names and state_dict shapes match torchvision's.

Tokens stay rows [B Hf Wf, C] in natural row-major order through the whole network.  The stem
is ``patchify`` (4 x 4) and the rows GEMM, then a row LayerNorm.  A block is pre-norm as in
``vit.py``: ``x + attn(norm1(x))`` and ``x + mlp(norm2(x))`` with ``residual_branch`` /
``residual_add``; the attention is ``Fn.window_attention``, which reads the in-projection's
rows where they lie: the cyclic shift, the window partition and its reverse are address
arithmetic inside the kernel, and the relative-position bias and the shift mask are computed
there, so no rolled, partitioned or padded copy of an activation is made.  Odd blocks shift
by window // 2, except where the map is no larger than the window.

Patch merging is ``patch_merge_rows`` (``patchify`` with P = 2, ``unpatchify`` backward) ->
LayerNorm(4 C) -> Linear(4 C, 2 C, bias=False).  ``patchify`` orders a 2 x 2 cell (ky, kx, c)
where torchvision concatenates (0,0), (1,0), (0,1), (1,1): the ``norm`` vectors and the
``reduction`` columns are permuted on import / export, not on the device.

Stochastic depth is not implemented: the model runs at rate 0 (torchvision's ``swin_t`` recipe
uses 0.2), as ConvNeXt here does.  The model is built for maps the window divides.

Swin-V2-T (torchvision ``swin_v2_t``, window 8 at 256 x 256) is the same network with three
parts exchanged.  The attention is ``ShiftedWindowAttentionV2``: cosine scores times a clamped
learned temperature, and a bias table that ``Fn.cpb_bias`` computes from a small MLP over
log-spaced offsets (``Fn.window_attention_cos``, the cosine variant of the same kernels).  The
block is residual-post-norm, ``x + norm1(attn(x))`` and ``x + norm2(mlp(x))``.  Patch merging
normalises after the reduction: rows -> Linear(4 C, 2 C, bias=False) -> LayerNorm(2 C), with the
same column permutation of ``reduction`` on import / export and a plain ``norm``.  Stochastic
depth is not implemented here either (rate 0; torchvision's ``swin_v2_t`` recipe uses 0.2).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops import functional as Fn
from .layers import (GELU, LayerNorm, Linear, PatchEmbed, ShiftedWindowAttention,
                     ShiftedWindowAttentionV2)


def _cells(t):
    """Swap the (0, 1) and (1, 0) blocks of the last axis' four C-wide blocks: torchvision's
    concat order <-> patchify's (ky, kx) order (its own inverse)."""
    c = t.shape[-1] // 4
    return t.reshape(*t.shape[:-1], 4, c)[..., [0, 2, 1, 3], :].reshape(t.shape)


class _MergeNorm(LayerNorm):
    def __init__(self, width: int):
        super().__init__(width, eps=1e-5)
        for p in (self.weight, self.bias):
            p._mpa_export = _cells
            p._mpa_import = _cells

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        for k in (prefix + "weight", prefix + "bias"):
            if k in destination:
                destination[k] = _cells(destination[k])

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for k in (prefix + "weight", prefix + "bias"):
            if k in state_dict:
                state_dict[k] = _cells(state_dict[k])
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class _MergeLinear(Linear):
    def __init__(self, dim: int):
        super().__init__(4 * dim, 2 * dim, bias=False)
        self.weight._mpa_export = self._exp
        self.weight._mpa_import = self._imp

    def _exp(self, t):
        return _cells(super()._exp(t))

    def _imp(self, t):
        return super()._imp(_cells(t))


class PatchMerging(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.dim = dim
        self.reduction = _MergeLinear(dim)
        self.norm = _MergeNorm(4 * dim)

    def forward(self, rows, B: int, Hf: int, Wf: int):
        """rows [B Hf Wf, C] -> [B Hf/2 Wf/2, 2 C]"""
        x = Fn.patch_merge_rows(rows.reshape(B, Hf, Wf, self.dim))
        return Fn.linear_act(self.norm(x), self.reduction)


class SwinBlock(nn.Module):
    attention = ShiftedWindowAttention

    def __init__(self, dim: int, heads: int, window: int, shift: int, mlp_ratio: float = 4.0):
        super().__init__()
        self.norm1 = LayerNorm(dim, eps=1e-5)
        self.attn = self.attention(dim, window, shift, heads)
        self.norm2 = LayerNorm(dim, eps=1e-5)
        hidden = int(dim * mlp_ratio)
        # torchvision's MLP indices: 2 and 4 are its dropouts
        self.mlp = nn.Sequential(Linear(dim, hidden), GELU(), nn.Identity(), Linear(hidden, dim),
                                 nn.Identity())

    def forward(self, rows, Hf: int, Wf: int):
        xb, join = Fn.residual_branch(rows)
        x = Fn.residual_add(self.attn(self.norm1(xb), Hf, Wf), rows, join)
        xb, join = Fn.residual_branch(x)
        h = Fn.linear_gelu(self.norm2(xb), self.mlp[0])
        return Fn.residual_add(Fn.linear_act(h, self.mlp[3]), x, join)


class PatchMergingV2(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.dim = dim
        self.reduction = _MergeLinear(dim)
        self.norm = LayerNorm(2 * dim, eps=1e-5)

    def forward(self, rows, B: int, Hf: int, Wf: int):
        """rows [B Hf Wf, C] -> [B Hf/2 Wf/2, 2 C]"""
        x = Fn.patch_merge_rows(rows.reshape(B, Hf, Wf, self.dim))
        return self.norm(Fn.linear_act(x, self.reduction))


class SwinBlockV2(SwinBlock):
    """Residual-post-norm: the LayerNorm follows the branch and its output is the residual
    add's in-place operand (the LayerNorm's backward reads its input, not its output)."""

    attention = ShiftedWindowAttentionV2

    def forward(self, rows, Hf: int, Wf: int):
        xb, join = Fn.residual_branch(rows)
        x = Fn.residual_add(self.norm1(self.attn(xb, Hf, Wf)), rows, join)
        xb, join = Fn.residual_branch(x)
        h = Fn.linear_gelu(xb, self.mlp[0])
        return Fn.residual_add(self.norm2(Fn.linear_act(h, self.mlp[3])), x, join)


class SwinTransformer(nn.Module):
    def __init__(self, patch: int = 4, width: int = 96, depths=(2, 2, 6, 2), heads=(3, 6, 12, 24),
                 window: int = 7, num_classes: int = 1000, block=SwinBlock, merge=PatchMerging):
        super().__init__()
        self.patch, self.width, self.window = patch, width, window
        # torchvision's indices: features.0 is (conv, permute, norm)
        layers = [nn.Sequential(PatchEmbed(3, width, patch), nn.Identity(), LayerNorm(width, eps=1e-5))]
        dim = width
        for s, (depth, nh) in enumerate(zip(depths, heads)):
            layers.append(nn.Sequential(*[block(dim, nh, window, 0 if i % 2 == 0 else window // 2)
                                          for i in range(depth)]))
            if s + 1 < len(depths):
                layers.append(merge(dim))
                dim *= 2
        self.features = nn.Sequential(*layers)
        self.norm = LayerNorm(dim, eps=1e-5)
        self.head = Linear(dim, num_classes)
        for m in self.modules():  # torchvision's init: truncated normal weights, zero biases
            if isinstance(m, Linear):
                m.init_(lambda w: nn.init.trunc_normal_(w, std=0.02))
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, x):
        B, P = x.shape[0], self.patch
        if x.shape[1] % P or x.shape[2] % P:
            raise ValueError("SwinTransformer: the image must be a multiple of the patch")
        Hf, Wf = x.shape[1] // P, x.shape[2] // P
        stem = self.features[0]
        rows = stem[2](Fn.linear_act(Fn.K(x).patchify(stem[0].fit_input(x), P), stem[0]))
        for m in list(self.features)[1:]:
            if isinstance(m, (PatchMerging, PatchMergingV2)):
                rows = m(rows, B, Hf, Wf)
                Hf, Wf = Hf // 2, Wf // 2
            else:
                for blk in m:
                    rows = blk(rows, Hf, Wf)
        rows = self.norm(rows)
        pooled = Fn.adaptive_avg_pool2d(rows.reshape(B, Hf, Wf, rows.shape[-1]), (1, 1))
        return self.head(pooled.reshape(B, -1))


def swin_t(num_classes: int = 1000) -> SwinTransformer:
    return SwinTransformer(num_classes=num_classes)


def swin_v2_t(num_classes: int = 1000) -> SwinTransformer:
    """torchvision's ``swin_v2_t``: patch 4, width 96, depths 2-2-6-2, heads 3-6-12-24, window 8
    (256 x 256 images: maps 64, 32, 16, 8)."""
    return SwinTransformer(window=8, num_classes=num_classes, block=SwinBlockV2, merge=PatchMergingV2)
