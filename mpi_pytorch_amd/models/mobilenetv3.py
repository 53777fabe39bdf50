"""MobileNetV3-Large (torchvision ``mobilenet_v3_large``): parameter names and OIHW shapes match
torchvision's state_dict.

Inverted-residual blocks: 1x1 expand -> depthwise k x k / s -> (squeeze-excite) -> 1x1 project,
each conv followed by BatchNorm; ReLU in the first six blocks, hardswish after.  The 1x1 convs
run on the rows GEMM and the depthwise conv on the ``dwconv`` kernels, both with their BN's
statistics from the epilogue; BN apply, hardswish, the SE pool / gate / scale and all their
backward passes are the ``se.hip`` kernel family (``Fn.bn_act_gate``), so the activated
expanded tensor is never stored.  ReLU layers without SE keep the fused BN kernels.
"""
from __future__ import annotations

import torch.nn as nn

from ..ops import functional as Fn
from .layers import (AdaptiveAvgPool2d, BatchNorm2d, Conv2d, Dropout, Hardswish, Linear, ReLU,
                     SqueezeExcitation)

# (in, kernel, expanded, out, squeeze-excite, hardswish, stride) of features.1 .. features.15
_BLOCKS = ((16, 3, 16, 16, False, False, 1), (16, 3, 64, 24, False, False, 2),
           (24, 3, 72, 24, False, False, 1), (24, 5, 72, 40, True, False, 2),
           (40, 5, 120, 40, True, False, 1), (40, 5, 120, 40, True, False, 1),
           (40, 3, 240, 80, False, True, 2), (80, 3, 200, 80, False, True, 1),
           (80, 3, 184, 80, False, True, 1), (80, 3, 184, 80, False, True, 1),
           (80, 3, 480, 112, True, True, 1), (112, 3, 672, 112, True, True, 1),
           (112, 5, 672, 160, True, True, 2), (160, 5, 960, 160, True, True, 1),
           (160, 5, 960, 160, True, True, 1))


def _make_divisible(v: float, divisor: int = 8) -> int:
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def _conv_bn(cin: int, cout: int, k: int, stride: int, act, groups: int = 1) -> nn.Sequential:
    """torchvision's Conv2dNormActivation: .0 conv, .1 BN, .2 the activation (no parameters)."""
    mods = [Conv2d(cin, cout, k, stride, k // 2, bias=False, groups=groups),
            BatchNorm2d(cout, eps=1e-3, momentum=0.01)]
    if act is not None:
        mods.append(Hardswish() if act == Fn.ACT_HARDSWISH else ReLU(inplace=True))
    return nn.Sequential(*mods)


class _InvertedResidual(nn.Module):
    def __init__(self, cin: int, k: int, exp: int, cout: int, use_se: bool, hs: bool, stride: int):
        super().__init__()
        self.act = Fn.ACT_HARDSWISH if hs else Fn.ACT_RELU
        self.use_res_connect = stride == 1 and cin == cout
        self.expand = exp != cin
        layers = [_conv_bn(cin, exp, 1, 1, self.act)] if self.expand else []
        layers.append(_conv_bn(exp, exp, k, stride, self.act, groups=exp))
        if use_se:
            layers.append(SqueezeExcitation(exp, _make_divisible(exp // 4, 8)))
        layers.append(_conv_bn(exp, cout, 1, 1, None))
        self.block = nn.Sequential(*layers)
        self.se_index = len(layers) - 2 if use_se else None

    def forward(self, x):
        b = self.block
        y, i = x, 0
        if self.expand:
            y, i = Fn.conv_bn_act_gate(x, b[0][0], b[0][1], self.act), 1
        se = b[self.se_index] if self.se_index is not None else None
        y = Fn.dwconv_bn_act_gate(y, b[i][0], b[i][1], self.act, se)
        return Fn.conv_bn_act(y, b[-1][0], b[-1][1], relu=False,
                              residual=x if self.use_res_connect else None)


class MobileNetV3(nn.Module):
    def __init__(self, num_classes: int = 1000, dropout: float = 0.2):
        super().__init__()
        mods = [_conv_bn(3, 16, 3, 2, Fn.ACT_HARDSWISH)]
        mods += [_InvertedResidual(*c) for c in _BLOCKS]
        mods.append(_conv_bn(160, 960, 1, 1, Fn.ACT_HARDSWISH))
        self.features = nn.Sequential(*mods)
        self.avgpool = AdaptiveAvgPool2d((1, 1))  # (no parameters: absent from state_dict)
        self.classifier = nn.Sequential(Linear(960, 1280), Hardswish(), Dropout(dropout, inplace=True),
                                        Linear(1280, num_classes))
        for m in self.modules():
            if isinstance(m, Conv2d):
                m.init_(lambda w: nn.init.kaiming_normal_(w, mode="fan_out"))
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, Linear):
                m.init_(lambda w: nn.init.normal_(w, 0, 0.01))
                nn.init.zeros_(m.bias)

    def forward(self, x):
        f = self.features
        x = Fn.conv_bn_act_gate(x, f[0][0], f[0][1], Fn.ACT_HARDSWISH)
        for i in range(1, 16):
            x = f[i](x)
        x = Fn.conv_bn_act_gate(x, f[16][0], f[16][1], Fn.ACT_HARDSWISH)
        x = self.avgpool(x)
        c = self.classifier
        x = Fn.hardswish(c[0](x.reshape(x.shape[0], -1)))
        return c[3](c[2](x))


def mobilenet_v3_large(num_classes: int = 1000) -> MobileNetV3:
    return MobileNetV3(num_classes)
