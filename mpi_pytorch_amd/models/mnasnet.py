"""MNASNet-1.0 (torchvision ``mnasnet1_0``, version-2 layout): parameter names and OIHW shapes
match torchvision's state_dict.

The network is inverted-residual blocks: 1x1 expand -> depthwise k x k / s -> 1x1 project,
each followed by BatchNorm, ReLU after the first two.  The 1x1 convs run on the rows GEMM
with BN statistics from its epilogue (``conv_bn_act``); the depthwise conv is the ``dwconv``
kernel family, which also produces its BN's statistics in its epilogue (``dwconv_bn_act``).
Plain ReLU throughout, so the fused BN kernels serve it unchanged.
"""
from __future__ import annotations

import torch.nn as nn

from ..ops import functional as Fn
from .layers import AdaptiveAvgPool2d, BatchNorm2d, Conv2d, Dropout, Linear, ReLU

_BN_MOMENTUM = 1 - 0.9997

# (in, out, kernel, stride, expansion, repeats) of layers.8 .. layers.13
_STACKS = ((16, 24, 3, 2, 3, 3), (24, 40, 5, 2, 3, 3), (40, 80, 5, 2, 6, 3),
           (80, 96, 3, 1, 6, 2), (96, 192, 5, 2, 6, 4), (192, 320, 3, 1, 6, 1))


def _bn(c: int) -> BatchNorm2d:
    return BatchNorm2d(c, momentum=_BN_MOMENTUM)


class _InvertedResidual(nn.Module):
    def __init__(self, cin: int, cout: int, k: int, stride: int, expansion: int):
        super().__init__()
        mid = cin * expansion
        self.apply_residual = cin == cout and stride == 1
        self.layers = nn.Sequential(
            Conv2d(cin, mid, 1, bias=False), _bn(mid), ReLU(inplace=True),
            Conv2d(mid, mid, k, stride, k // 2, bias=False, groups=mid), _bn(mid),
            ReLU(inplace=True),
            Conv2d(mid, cout, 1, bias=False), _bn(cout))

    def forward(self, x):
        m = self.layers
        y = Fn.conv_bn_act(x, m[0], m[1], relu=True)
        y = Fn.dwconv_bn_act(y, m[3], m[4], relu=True)
        return Fn.conv_bn_act(y, m[6], m[7], relu=False,
                              residual=x if self.apply_residual else None)


def _stack(cin, cout, k, stride, expansion, repeats) -> nn.Sequential:
    blocks = [_InvertedResidual(cin, cout, k, stride, expansion)]
    blocks += [_InvertedResidual(cout, cout, k, 1, expansion) for _ in range(1, repeats)]
    return nn.Sequential(*blocks)


class MNASNet(nn.Module):
    def __init__(self, num_classes: int = 1000, dropout: float = 0.2):
        super().__init__()
        mods = [Conv2d(3, 32, 3, 2, 1, bias=False), _bn(32), ReLU(inplace=True),
                Conv2d(32, 32, 3, 1, 1, bias=False, groups=32), _bn(32), ReLU(inplace=True),
                Conv2d(32, 16, 1, bias=False), _bn(16)]
        mods += [_stack(*s) for s in _STACKS]
        mods += [Conv2d(320, 1280, 1, bias=False), _bn(1280), ReLU(inplace=True)]
        self.layers = nn.Sequential(*mods)
        self.avgpool = AdaptiveAvgPool2d((1, 1))  # (no parameters: absent from state_dict)
        self.classifier = nn.Sequential(Dropout(dropout, inplace=True), Linear(1280, num_classes))
        for m in self.modules():
            if isinstance(m, Conv2d):
                m.init_(lambda w: nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu"))
            elif isinstance(m, Linear):
                m.init_(lambda w: nn.init.kaiming_uniform_(w, mode="fan_out",
                                                            nonlinearity="sigmoid"))
                nn.init.zeros_(m.bias)

    def forward(self, x):
        m = self.layers
        x = Fn.conv_bn_act(x, m[0], m[1], relu=True)
        x = Fn.dwconv_bn_act(x, m[3], m[4], relu=True)
        x = Fn.conv_bn_act(x, m[6], m[7], relu=False)
        for i in range(8, 14):
            for blk in m[i]:
                x = blk(x)
        x = Fn.conv_bn_act(x, m[14], m[15], relu=True)
        x = self.avgpool(x)
        return self.classifier(x.reshape(x.shape[0], -1))


def mnasnet1_0(num_classes: int = 1000) -> MNASNet:
    return MNASNet(num_classes)
