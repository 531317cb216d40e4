"""DeepLabV3+ on a MobileNetV2 backbone in "fabu" style (Chen et al. 2018; the backbone of model/mobilenetv2/MobileNetV2_fabu.py
without its 1x1 to 1280 channels and its head).

  backbone   the stem and the seventeen inverted residual blocks; once the running stride has reached `output_stride` (16 or 8)
             every further stride-2 block keeps stride 1 and it and the blocks behind it dilate their depthwise 3x3 instead
             (padding = dilation): the last four depthwise layers at output stride 16 (dilation 2), the last eleven at 8
             (dilation 2, then 4)
  ASPP       on the backbone's output (320 * width_mult channels): a 1x1 branch and three atrous SEPARABLE branches (depthwise
             3x3 at rate 6 / 12 / 18, at output stride 8 at 12 / 24 / 36, padding = rate -> BN -> ReLU -> 1x1 -> BN -> ReLU), each to
             `head_width` channels, joined by nested Concats and projected 1x1 back to `head_width` (256)
  decoder    nn.Upsample(bilinear) by output_stride / 4 (x4 at output stride 16) up to the stride-4 plane -> a 1x1 projection of
             the stride-4 features to `low_width` (48) channels -> Concat(up, low) -> two 3x3 convolutions to `head_width` -> the
             1x1 classifier -> nn.Upsample(bilinear, x4) to the input's size: logits [N, num_classes, input_size, input_size]

The image-pooling branch of the paper's ASPP is LEFT OUT: its adaptive average pool and its `size=` upsampling are foreign to
the resident plan (a global value broadcast over the plane has no int8 NHWC form here), and a network with it would leave the
integers in the middle of the ASPP whatever else is planned.  The dropouts are left out too (identity at inference).

Every join is a Concat marker, every upsampling an nn.Upsample module and every activation out of place, so forward hooks see
each cared tensor and merge_bn -> Quantity -> Reconstruction.ReconModel take the model as it stands.  With
resident.enable(..., depthwise=True, relu6=True, concat=True, flatten=True, bilinear=True, requant=True) everything between the
stem and the logits stays int8 except the atrous depthwise layers; those join where NewConv2d.use_atrous_i8 is set
(fq_dwconv2d_dil_i8_resident, scripts/atrous_cost.py).

The reference ships no DeepLab; this one is written from the architecture.  `width_mult` scales the backbone and, below 1, the
head's two widths with it (tests build a narrow network); `input_size` must be a multiple of 32.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Concat, Eltwise  # noqa: E402

STEM_WIDTH = 32
# (expansion factor t, output width c, repeats n, stride of the first repeat s): table 2 of the MobileNetV2 paper
STAGES = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
ASPP_RATES = {16: (6, 12, 18), 8: (12, 24, 36)}


def make_divisible(v, divisor=8):
    new = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new + divisor if new < 0.9 * v else new


def _conv_bn_act(cin, cout, k, stride=1, dilation=1, groups=1, act=nn.ReLU):
    """conv (padding keeps the plane at stride 1: dilation * (k // 2)) -> BN -> act (None: linear)."""
    layers = [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=dilation * (k // 2), dilation=dilation, groups=groups,
                        bias=False), nn.BatchNorm2d(cout)]
    if act is not None:
        layers.append(act(False))
    return nn.Sequential(*layers)


class InvertedResidual(nn.Module):
    """project(relu6(dw(relu6(expand(x))))), the depthwise 3x3 at `dilation`; with a shortcut Eltwise(that, x)."""

    def __init__(self, inchannel, outchannel, stride, expand, dilation):
        super(InvertedResidual, self).__init__()
        hidden = inchannel * expand
        self.expand = _conv_bn_act(inchannel, hidden, 1, act=nn.ReLU6) if expand != 1 else None
        self.dw = _conv_bn_act(hidden, hidden, 3, stride, dilation, groups=hidden, act=nn.ReLU6)
        self.project = _conv_bn_act(hidden, outchannel, 1, act=None)
        self.Eltwise = Eltwise() if (stride == 1 and inchannel == outchannel) else None

    def forward(self, x):
        y = x if self.expand is None else self.expand(x)
        y = self.project(self.dw(y))
        if self.Eltwise is not None:
            y = self.Eltwise(y, x)
        return y


class AtrousSeparable(nn.Sequential):
    """depthwise 3x3 at `rate` -> BN -> ReLU -> 1x1 -> BN -> ReLU"""

    def __init__(self, cin, cout, rate):
        super(AtrousSeparable, self).__init__(_conv_bn_act(cin, cin, 3, dilation=rate, groups=cin), _conv_bn_act(cin, cout, 1))


class DeepLabV3Plus(nn.Module):

    def __init__(self, num_classes=21, output_stride=16, width_mult=1.0, input_size=224, head_width=256, low_width=48):
        super(DeepLabV3Plus, self).__init__()
        if output_stride not in ASPP_RATES:
            raise ValueError("DeepLabV3Plus: output_stride must be 16 or 8, got %r" % (output_stride,))
        if input_size < 32 or input_size % 32:
            raise ValueError("DeepLabV3Plus: input_size must be a multiple of 32, got %r" % (input_size,))
        scale = min(1.0, width_mult)
        head_width, low_width = make_divisible(head_width * scale), make_divisible(low_width * scale)
        width = make_divisible(STEM_WIDTH * width_mult)
        self.conv1 = _conv_bn_act(3, width, 3, stride=2, act=nn.ReLU6)
        low, high = nn.Sequential(), nn.Sequential()          # the blocks up to the stride-4 features, and the ones behind
        reduction, dilation = 2, 1
        for (t, c, n, s) in STAGES:
            out = make_divisible(c * width_mult)
            for i in range(n):
                stride = s if i == 0 else 1
                if stride == 2 and reduction == output_stride:
                    stride, dilation = 1, dilation * 2        # the stride becomes dilation, from this block on
                reduction *= stride
                part = low if c <= 24 else high               # (the first two stages: stride 4, never dilated)
                part.add_module(str(len(part)), InvertedResidual(width, out, stride, t, dilation))
                width = out
            if c == 24:
                low_channels = width
        self.low_blocks, self.high_blocks = low, high
        self.aspp0 = _conv_bn_act(width, head_width, 1)
        self.aspp = nn.ModuleList(AtrousSeparable(width, head_width, r) for r in ASPP_RATES[output_stride])
        self.aspp_cats = nn.ModuleList(Concat() for _ in self.aspp)
        self.aspp_project = _conv_bn_act((1 + len(self.aspp)) * head_width, head_width, 1)
        self.up_aspp = nn.Upsample(scale_factor=output_stride // 4, mode="bilinear", align_corners=False)
        self.low_project = _conv_bn_act(low_channels, low_width, 1)
        self.Concat = Concat()
        self.decoder = nn.Sequential(_conv_bn_act(head_width + low_width, head_width, 3), _conv_bn_act(head_width, head_width, 3))
        self.classifier = nn.Conv2d(head_width, num_classes, kernel_size=1)
        self.up_logits = nn.Upsample(scale_factor=4, mode="bilinear", align_corners=False)

    def forward(self, x):
        low = self.low_blocks(self.conv1(x))
        high = self.high_blocks(low)
        y = self.aspp0(high)
        for branch, cat in zip(self.aspp, self.aspp_cats):
            y = cat(y, branch(high))
        y = self.up_aspp(self.aspp_project(y))
        y = self.Concat(y, self.low_project(low))
        return self.up_logits(self.classifier(self.decoder(y)))
