"""PVT v2 B2 (the official ``pvt_v2_b2``): parameter names and state_dict shapes match the
official implementation's, so its checkpoints load.

Tokens stay NHWC maps [B, Hf, Wf, C] through the whole network: a LayerNorm, a rows GEMM or
the attention reads them as rows [B Hf Wf, C], a conv as an image, and no permute exists.
Every stage opens with an overlapping patch embedding (a strided conv through ``Fn.conv_act``:
7 x 7 / 4 on the image, then 3 x 3 / 2) and a LayerNorm, and closes with ``norm{i}``.  A block is
pre-norm, ``x + attn(norm1(x))`` and ``x + mlp(norm2(x))`` with ``residual_branch`` /
``residual_add``.  The attention is ``SpatialReductionAttention``: all tokens are queries, keys
and values come from the map reduced by ``sr`` (kernel = stride = 8, 4, 2; none at stage 4) and
a LayerNorm: 7 x 7 = 49 tokens at every stage of a 224 x 224 image, which
``Fn.cross_attention`` keeps resident.  ``sr`` runs as ``Fn.patch_rows`` and the rows GEMM (the
strided-conv dgrad stops at 16 stride phases), so the image must be a multiple of 32; images
above 256 x 256 give more than 64 keys and are refused.  The MLP is fc1 -> 3 x 3 depthwise conv -> GELU -> fc2; the conv runs bias-free and
``Fn.dwconv_gelu`` adds its bias inside the GELU kernel.

LayerNorm eps is 1e-6 for ``norm1``, ``norm2`` and ``norm{i}`` and 1e-5 for the patch
embeddings' and the reductions' norms, as in the official code.  Stochastic depth is not
implemented: the model runs at rate 0 (the official B2 recipe uses 0.1), as ConvNeXt and Swin
here do.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from ..ops import functional as Fn
from .layers import Conv2d, LayerNorm, Linear, PatchEmbed, SpatialReductionAttention


class OverlapPatchEmbed(nn.Module):
    def __init__(self, in_channels: int, dim: int, kernel: int, stride: int):
        super().__init__()
        self.proj = Conv2d(in_channels, dim, kernel, stride=stride, padding=kernel // 2)
        self.norm = LayerNorm(dim, eps=1e-5)

    def forward(self, x):
        return self.norm(Fn.conv_act(x, self.proj))


class DWConv(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.dwconv = Conv2d(dim, dim, 3, stride=1, padding=1, bias=True, groups=dim)


class Mlp(nn.Module):
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.fc1 = Linear(dim, hidden)
        self.dwconv = DWConv(hidden)
        self.fc2 = Linear(hidden, dim)

    def forward(self, x):
        B, Hf, Wf, D = x.shape
        h = Fn.linear_act(x.reshape(B * Hf * Wf, D), self.fc1).reshape(B, Hf, Wf, -1)
        h = Fn.dwconv_gelu(h, self.dwconv.dwconv)
        return Fn.linear_act(h.reshape(B * Hf * Wf, -1), self.fc2).reshape(B, Hf, Wf, D)


class PVTBlock(nn.Module):
    def __init__(self, dim: int, heads: int, mlp_ratio: int, sr_ratio: int):
        super().__init__()
        self.norm1 = LayerNorm(dim, eps=1e-6)
        self.attn = SpatialReductionAttention(dim, heads, sr_ratio)
        self.norm2 = LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, dim * mlp_ratio)

    def forward(self, x):
        xb, join = Fn.residual_branch(x)
        x = Fn.residual_add(self.attn(self.norm1(xb)), x, join)
        xb, join = Fn.residual_branch(x)
        return Fn.residual_add(self.mlp(self.norm2(xb)), x, join)


class PyramidVisionTransformerV2(nn.Module):
    def __init__(self, widths=(64, 128, 320, 512), depths=(3, 4, 6, 3), heads=(1, 2, 5, 8),
                 mlp_ratios=(8, 8, 4, 4), sr_ratios=(8, 4, 2, 1), num_classes: int = 1000):
        super().__init__()
        self.stages = len(widths)
        cin = 3
        for s, (dim, depth, nh, mr, sr) in enumerate(zip(widths, depths, heads, mlp_ratios, sr_ratios)):
            setattr(self, "patch_embed%d" % (s + 1),
                    OverlapPatchEmbed(cin, dim, 7 if s == 0 else 3, 4 if s == 0 else 2))
            setattr(self, "block%d" % (s + 1),
                    nn.ModuleList([PVTBlock(dim, nh, mr, sr) for _ in range(depth)]))
            setattr(self, "norm%d" % (s + 1), LayerNorm(dim, eps=1e-6))
            cin = dim
        self.head = Linear(widths[-1], num_classes)
        for m in self.modules():  # the official init
            if isinstance(m, Linear):
                m.init_(lambda w: nn.init.trunc_normal_(w, std=0.02))
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, Conv2d):
                kh, kw = m.kernel_size
                std = math.sqrt(2.0 / (kh * kw * m.out_channels // m.groups))
                m.init_(lambda w, std=std: nn.init.normal_(w, 0.0, std))
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, PatchEmbed):  # the reductions: a conv's init, fan_out = P P width
                w = torch.empty(m.out_features, m.in_channels, m.patch, m.patch)
                w.normal_(0.0, math.sqrt(2.0 / (m.patch * m.patch * m.out_features)))
                with torch.no_grad():
                    m.weight.copy_(m._imp(w))

    def forward(self, x):
        for s in range(1, self.stages + 1):
            x = getattr(self, "patch_embed%d" % s)(x)
            for blk in getattr(self, "block%d" % s):
                x = blk(x)
            x = getattr(self, "norm%d" % s)(x)
        pooled = Fn.adaptive_avg_pool2d(x, (1, 1))
        return self.head(pooled.reshape(x.shape[0], -1))


def pvt_v2_b2(num_classes: int = 1000) -> PyramidVisionTransformerV2:
    """The official ``pvt_v2_b2``: widths 64-128-320-512, depths 3-4-6-3, heads 1-2-5-8, MLP
    ratios 8-8-4-4, reduction ratios 8-4-2-1 (224 x 224 images: maps 56, 28, 14, 7)."""
    return PyramidVisionTransformerV2(num_classes=num_classes)
