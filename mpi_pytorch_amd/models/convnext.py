"""ConvNeXt-Tiny (torchvision ``convnext_tiny``): parameter names and state_dict shapes match
torchvision's.

A block is 7x7 depthwise conv (with bias) -> LayerNorm over channels -> Linear C -> 4C -> GELU ->
Linear 4C -> C -> layer scale -> residual add.  On the kernels: the depthwise conv runs bias-free
and the LayerNorm kernel adds its bias in registers (``dwconv_ln``); the two Linears are the rows
GEMM over [N H W, C] (NHWC needs no permute), the first with the GELU backward reducing its
bias gradient (``linear_gelu``); layer scale and residual are one pass (``scale_residual``),
whose residual gradient reaches the block input through the depthwise dgrad's accumulate
operand (``GradJoin``).  Stem and downsamples are patchify convs (4x4/s4, 2x2/s2) on the
implicit GEMM.  Stochastic depth is not implemented: the model runs at rate 0.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops import functional as Fn
from .layers import AdaptiveAvgPool2d, Conv2d, Flatten, GELU, LayerNorm, Linear


class CNBlock(nn.Module):
    def __init__(self, dim: int, layer_scale: float = 1e-6):
        super().__init__()
        # torchvision's indices: 1 and 6 are its NCHW <-> NHWC permutes
        self.block = nn.Sequential(
            Conv2d(dim, dim, 7, 1, 3, bias=True, groups=dim), nn.Identity(), LayerNorm(dim),
            Linear(dim, 4 * dim), GELU(), Linear(4 * dim, dim), nn.Identity())
        # stored [C] (a per-channel scale like a norm's weight: 1-D for the weight-decay
        # exclusion), [C, 1, 1] in the state_dict
        self.layer_scale = nn.Parameter(torch.full((dim,), float(layer_scale)))
        self.layer_scale._mpa_export = self._exp_scale
        self.layer_scale._mpa_import = self._imp_scale

    @staticmethod
    def _exp_scale(t):
        return t.reshape(-1, 1, 1)

    @staticmethod
    def _imp_scale(t):
        return t.reshape(-1)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        k = prefix + "layer_scale"
        if k in destination:
            destination[k] = destination[k].reshape(-1, 1, 1)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = prefix + "layer_scale"
        if k in state_dict and state_dict[k].dim() == 3:
            state_dict[k] = state_dict[k].reshape(-1)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x):
        m = self.block
        join = Fn.GradJoin(2) if torch.is_grad_enabled() and x.requires_grad else None
        y = Fn.dwconv_ln(x, m[0], m[2], join=join)
        h = Fn.linear_gelu(y.reshape(-1, y.shape[-1]), m[3])
        # (a width that is no multiple of 32 is stored padded by Linear: its output is a column
        # slice, copied here; ConvNeXt's own widths are not)
        z = Fn.linear_act(h, m[5]).reshape(x.shape).contiguous()
        return Fn.scale_residual(z, self.layer_scale, x, join=join)


class ConvNeXt(nn.Module):
    def __init__(self, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), num_classes: int = 1000,
                 layer_scale: float = 1e-6):
        super().__init__()
        feats = [nn.Sequential(Conv2d(3, dims[0], 4, 4, 0, bias=True), LayerNorm(dims[0]))]
        for i, (depth, dim) in enumerate(zip(depths, dims)):
            feats.append(nn.Sequential(*[CNBlock(dim, layer_scale) for _ in range(depth)]))
            if i + 1 < len(dims):
                feats.append(nn.Sequential(LayerNorm(dim), Conv2d(dim, dims[i + 1], 2, 2, 0, bias=True)))
        self.features = nn.Sequential(*feats)
        self.avgpool = AdaptiveAvgPool2d((1, 1))
        self.classifier = nn.Sequential(LayerNorm(dims[-1]), Flatten(), Linear(dims[-1], num_classes))
        for m in self.modules():
            if isinstance(m, (Conv2d, Linear)):
                m.init_(lambda w: nn.init.trunc_normal_(w, std=0.02))
                nn.init.zeros_(m.bias)

    def forward(self, x):
        f = self.features
        x = f[0][1](Fn.conv_act(x, f[0][0]))
        for stage in list(f)[1:]:
            if isinstance(stage[0], LayerNorm):  # downsample
                x = Fn.conv_act(stage[0](x), stage[1])
            else:
                for blk in stage:
                    x = blk(x)
        x = self.classifier[0](self.avgpool(x))
        return self.classifier[2](x.reshape(x.shape[0], -1))


def convnext_tiny(num_classes: int = 1000) -> ConvNeXt:
    return ConvNeXt(num_classes=num_classes)
