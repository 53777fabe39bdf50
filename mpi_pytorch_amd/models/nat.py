"""NAT-Mini (the official ``nat_mini``): parameter names and state_dict shapes match the official
implementation's, so its checkpoints load.

The tokenizer is two biased 3 x 3 / 2 convs (``Fn.conv_act``) and a LayerNorm; tokens are then
rows [B Hf Wf, C] in natural order, which a conv reads as an NHWC map by a reshape.  A block is
pre-norm, ``x + attn(norm1(x))`` and ``x + mlp(norm2(x))`` with ``residual_branch`` /
``residual_add``; the attention is ``layers.NeighborhoodAttention`` (``Fn.neighborhood_attention``
on ``nattn.hip``: every pixel attends the 7 x 7 neighbourhood centred on it, clamped to the
map), the MLP ``Fn.linear_gelu`` and a rows GEMM.  Between levels a bias-free 3 x 3 / 2 conv
doubles the width and a LayerNorm follows.  Then ``norm``, the token mean and ``head``.

Every level's map must be at least 7 x 7: with four levels, images are multiples of 32 and at
least 224 x 224.  LayerNorm eps is 1e-5.  Stochastic depth is not implemented: the model runs at
rate 0 (the official recipe uses 0.2), as the other transformer models here do.
"""
from __future__ import annotations

import torch.nn as nn

from ..ops import functional as Fn
from .layers import Conv2d, LayerNorm, Linear, NeighborhoodAttention


class ConvTokenizer(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.proj = nn.Sequential(Conv2d(3, dim // 2, 3, stride=2, padding=1),
                                  Conv2d(dim // 2, dim, 3, stride=2, padding=1))
        self.norm = LayerNorm(dim, eps=1e-5)

    def forward(self, x):
        return self.norm(Fn.conv_act(Fn.conv_act(x, self.proj[0]), self.proj[1]))


class ConvDownsampler(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.reduction = Conv2d(dim, 2 * dim, 3, stride=2, padding=1, bias=False)
        self.norm = LayerNorm(2 * dim, eps=1e-5)

    def forward(self, x):
        return self.norm(Fn.conv_act(x, self.reduction))


class Mlp(nn.Module):
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.fc1 = Linear(dim, hidden)
        self.fc2 = Linear(hidden, dim)

    def forward(self, rows):
        return Fn.linear_act(Fn.linear_gelu(rows, self.fc1), self.fc2)


class NATBlock(nn.Module):
    def __init__(self, dim: int, heads: int, mlp_ratio: float):
        super().__init__()
        self.norm1 = LayerNorm(dim, eps=1e-5)
        self.attn = NeighborhoodAttention(dim, heads)
        self.norm2 = LayerNorm(dim, eps=1e-5)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    def forward(self, rows, Hf: int, Wf: int):
        xb, join = Fn.residual_branch(rows)
        x = Fn.residual_add(self.attn(self.norm1(xb), Hf, Wf), rows, join)
        xb, join = Fn.residual_branch(x)
        return Fn.residual_add(self.mlp(self.norm2(xb)), x, join)


class NATLevel(nn.Module):
    def __init__(self, dim: int, depth: int, heads: int, mlp_ratio: float, downsample: bool):
        super().__init__()
        self.blocks = nn.ModuleList([NATBlock(dim, heads, mlp_ratio) for _ in range(depth)])
        if downsample:
            self.downsample = ConvDownsampler(dim)

    def forward(self, x):
        """map [B, Hf, Wf, C] -> [B, ceil(Hf / 2), ceil(Wf / 2), 2 C] (the last level keeps its map)"""
        B, Hf, Wf, C = x.shape
        rows = x.reshape(B * Hf * Wf, C)
        for blk in self.blocks:
            rows = blk(rows, Hf, Wf)
        x = rows.reshape(B, Hf, Wf, C)
        return self.downsample(x) if hasattr(self, "downsample") else x


class NAT(nn.Module):
    def __init__(self, width: int = 64, depths=(3, 4, 6, 5), heads=(2, 4, 8, 16), mlp_ratio: float = 3.0,
                 num_classes: int = 1000):
        super().__init__()
        self.patch_embed = ConvTokenizer(width)
        n = len(depths)
        self.levels = nn.ModuleList([NATLevel(width << i, depths[i], heads[i], mlp_ratio, i + 1 < n)
                                     for i in range(n)])
        self.norm = LayerNorm(width << (n - 1), eps=1e-5)
        self.head = Linear(width << (n - 1), num_classes)
        for m in self.modules():  # the official init: truncated normal weights, zero biases
            if isinstance(m, Linear):
                m.init_(lambda w: nn.init.trunc_normal_(w, std=0.02))
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, x):
        cut = 4 << (len(self.levels) - 1)
        if x.shape[1] % cut or x.shape[2] % cut or min(x.shape[1], x.shape[2]) < 7 * cut:
            raise ValueError("NAT: the image must be a multiple of {} and at least {} x {} (a 7 x 7 "
                             "last map)".format(cut, 7 * cut, 7 * cut))
        x = self.patch_embed(x)
        for level in self.levels:
            x = level(x)
        B, Hf, Wf, C = x.shape
        rows = self.norm(x.reshape(B * Hf * Wf, C))
        pooled = Fn.adaptive_avg_pool2d(rows.reshape(B, Hf, Wf, C), (1, 1))
        return self.head(pooled.reshape(B, -1))


def nat_mini(num_classes: int = 1000) -> NAT:
    """The official ``nat_mini``: widths 64-128-256-512, depths 3-4-6-5, heads 2-4-8-16, MLP ratio
    3, neighbourhood 7 (224 x 224 images: maps 56, 28, 14, 7)."""
    return NAT(num_classes=num_classes)
