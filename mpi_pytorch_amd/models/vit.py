"""ViT-B/16 (torchvision ``vit_b_16``): parameter names and state_dict shapes match
torchvision's.

The image becomes patch rows (``patchify``), the patch embedding is the rows GEMM, and the
class token and position embedding are added in one pass (``Fn.patch_tokens``).  The encoder
keeps the tokens as rows [B S, D] throughout: LayerNorm, the in-projection, the out-projection
and the MLP are row kernels, and the attention kernels read the in-projection's rows as the
packed [B, S, 3, H, 64] buffer and write the out-projection's rows, so nothing is permuted.  A
pre-norm block is ``x + f(ln(x))``: the branch output is added to in place (``residual_add``)
and the two gradients of x meet in a ``GradJoin``.  The class token's row alone goes through
the final ``encoder.ln`` (LayerNorm is per row) and the head.  Dropout rates are 0 as in
torchvision's default, so no dropout module runs; the model is built for one image size.
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as nn

from ..ops import functional as Fn
from .layers import GELU, LayerNorm, Linear, MultiheadAttention, PatchEmbed


def _flat(t):
    return t.reshape(-1)


def _token(t):
    return t.reshape(1, 1, -1)


class EncoderBlock(nn.Module):
    def __init__(self, heads: int, width: int, mlp: int):
        super().__init__()
        self.ln_1 = LayerNorm(width, eps=1e-6)
        self.self_attention = MultiheadAttention(width, heads)
        self.ln_2 = LayerNorm(width, eps=1e-6)
        # torchvision's MLPBlock indices: 2 and 4 are its dropouts
        self.mlp = nn.Sequential(Linear(width, mlp), GELU(), nn.Identity(), Linear(mlp, width),
                                 nn.Identity())
        for m in (self.mlp[0], self.mlp[3]):
            m.init_(nn.init.xavier_uniform_)
            nn.init.normal_(m.bias, std=1e-6)

    def forward(self, rows, B: int, S: int):
        xb, join = Fn.residual_branch(rows)
        x = Fn.residual_add(self.self_attention(self.ln_1(xb), B, S), rows, join)
        xb, join = Fn.residual_branch(x)
        h = Fn.linear_gelu(self.ln_2(xb), self.mlp[0])
        return Fn.residual_add(Fn.linear_act(h, self.mlp[3]), x, join)


class Encoder(nn.Module):
    def __init__(self, seq: int, depth: int, heads: int, width: int, mlp: int):
        super().__init__()
        self.seq, self.width = seq, width
        # stored flat (1-D: left out of weight decay and trust ratio like a norm's parameters,
        # as torchvision's recipe does), [1, S, D] in the state_dict
        self.pos_embedding = nn.Parameter(torch.empty(seq * width).normal_(std=0.02))
        self.pos_embedding._mpa_export = self._exp_pos
        self.pos_embedding._mpa_import = _flat
        self.layers = nn.Sequential(OrderedDict(
            ("encoder_layer_%d" % i, EncoderBlock(heads, width, mlp)) for i in range(depth)))
        self.ln = LayerNorm(width, eps=1e-6)

    def _exp_pos(self, t):
        return t.reshape(1, self.seq, self.width)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        k = prefix + "pos_embedding"
        if k in destination:
            destination[k] = destination[k].reshape(1, self.seq, self.width)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = prefix + "pos_embedding"
        if k in state_dict and state_dict[k].dim() == 3:
            state_dict[k] = state_dict[k].reshape(-1)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class VisionTransformer(nn.Module):
    def __init__(self, image_size: int = 224, patch: int = 16, depth: int = 12, heads: int = 12,
                 width: int = 768, mlp: int = 3072, num_classes: int = 1000):
        super().__init__()
        if image_size % patch:
            raise ValueError("VisionTransformer: image_size must be a multiple of the patch")
        self.image_size, self.patch, self.width = image_size, patch, width
        self.seq = (image_size // patch) ** 2 + 1
        self.class_token = nn.Parameter(torch.zeros(width))  # [1, 1, D] in the state_dict
        self.class_token._mpa_export = _token
        self.class_token._mpa_import = _flat
        self.conv_proj = PatchEmbed(3, width, patch)
        self.encoder = Encoder(self.seq, depth, heads, width, mlp)
        head = Linear(width, num_classes)
        head.init_(nn.init.zeros_)
        nn.init.zeros_(head.bias)
        self.heads = nn.Sequential(OrderedDict(head=head))

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        k = prefix + "class_token"
        if k in destination:
            destination[k] = destination[k].reshape(1, 1, -1)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = prefix + "class_token"
        if k in state_dict and state_dict[k].dim() == 3:
            state_dict[k] = state_dict[k].reshape(-1)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x):
        if x.shape[1] != self.image_size or x.shape[2] != self.image_size:
            raise ValueError("VisionTransformer: built for %d x %d images, got %d x %d"
                             % (self.image_size, self.image_size, x.shape[1], x.shape[2]))
        B, S, D = x.shape[0], self.seq, self.width
        tok = Fn.patch_tokens(self.conv_proj.fit_input(x), self.conv_proj, self.class_token,
                              self.encoder.pos_embedding)
        rows = tok.reshape(B * S, D)
        for blk in self.encoder.layers:
            rows = blk(rows, B, S)
        cls = rows.reshape(B, S, D)[:, 0].contiguous()
        return self.heads.head(self.encoder.ln(cls))


def vit_b_16(num_classes: int = 1000) -> VisionTransformer:
    return VisionTransformer(num_classes=num_classes)
