"""MobileNetV2 in "fabu" style: a 3x3 stem (stride 2), seventeen inverted residual blocks (1x1 expansion -> BN -> ReLU6 ->
depthwise 3x3 -> BN -> ReLU6 -> linear 1x1 projection -> BN, no activation behind it), a 1x1 to 1280 channels -> BN -> ReLU6, a
global average pool and a Linear classifier.  A block whose stride is 1 and whose input and output widths match adds its input
back through the marker module Eltwise, and nothing follows the add; the flatten is the marker module View; every activation is
an out-of-place nn.ReLU6(False), so forward hooks see each cared tensor and merge_bn -> Quantity -> Reconstruction.ReconModel
take the model as it stands (tools/configs.yml lists ReLU6 among the traced op types).

The reference ships no MobileNetV2; this one is written from the architecture (Sandler et al. 2018, table 2), in the style of
model/mobilenet/MobileNet_fabu.py.  It is the model the fused ReLU6 is measured on (scripts/relu6_cost.py): resident.enable(...,
depthwise=True, relu6=True) runs every expansion, depthwise and stem layer with its ReLU6 as one integer kernel, and
Quantity.fuse_relu6 lets the calibration forward's own convolutions write the clipped copy.

`width_mult` scales every width (rounded to a multiple of `divisor`, never below it and never by more than 10 % down, as the
paper's code does); `input_size` must be a multiple of 32; `stages` / `last_width` replace table 2 (tests build a small network
with them); `batch_norm=False` builds the network as merge_bn leaves it (convolutions with a bias, no BatchNorm), which is what
tests with hand-made integer weights want.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Eltwise, View  # noqa: E402

STEM_WIDTH = 32
LAST_WIDTH = 1280
# (expansion factor t, output width c, repeats n, stride of the first repeat s): table 2 of the paper
STAGES = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))


def make_divisible(v, divisor=8):
    new = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new + divisor if new < 0.9 * v else new


def _conv_bn(cin, cout, k, stride, pad, groups=1, batch_norm=True):
    if not batch_norm:
        return [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad, groups=groups, bias=True)]
    return [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad, groups=groups, bias=False), nn.BatchNorm2d(cout)]


class InvertedResidual(nn.Module):
    """project(relu6(dw(relu6(expand(x))))), with t == 1 no expansion layer; with a shortcut Eltwise(that, x)."""

    def __init__(self, inchannel, outchannel, stride, expand, batch_norm=True):
        super(InvertedResidual, self).__init__()
        hidden = inchannel * expand
        if expand != 1:
            self.expand = nn.Sequential(*_conv_bn(inchannel, hidden, 1, 1, 0, batch_norm=batch_norm), nn.ReLU6(False))
        else:
            self.expand = None
        self.dw = nn.Sequential(*_conv_bn(hidden, hidden, 3, stride, 1, groups=hidden, batch_norm=batch_norm), nn.ReLU6(False))
        self.project = nn.Sequential(*_conv_bn(hidden, outchannel, 1, 1, 0, batch_norm=batch_norm))
        self.Eltwise = Eltwise() if (stride == 1 and inchannel == outchannel) else None

    def forward(self, x):
        y = x if self.expand is None else self.expand(x)
        y = self.project(self.dw(y))
        if self.Eltwise is not None:
            y = self.Eltwise(y, x)
        return y


class MobileNetV2(nn.Module):

    def __init__(self, num_classes=1000, width_mult=1.0, input_size=224, divisor=8, stages=STAGES, last_width=LAST_WIDTH,
                 batch_norm=True):
        super(MobileNetV2, self).__init__()
        width = make_divisible(STEM_WIDTH * width_mult, divisor)
        self.conv1 = nn.Sequential(*_conv_bn(3, width, 3, 2, 1, batch_norm=batch_norm), nn.ReLU6(False))
        blocks = nn.Sequential()
        reduction = 2
        for (t, c, n, s) in stages:
            out = make_divisible(c * width_mult, divisor)
            for i in range(n):
                stride = s if i == 0 else 1
                blocks.add_module(str(len(blocks)), InvertedResidual(width, out, stride, t, batch_norm))
                reduction *= stride
                width = out
        self.blocks = blocks
        assert input_size % reduction == 0, "the input size must be a multiple of the stride-2 layers' product, %d" % reduction
        last = make_divisible(last_width * max(1.0, width_mult), divisor)    # (the last layer is never made narrower)
        self.conv_last = nn.Sequential(*_conv_bn(width, last, 1, 1, 0, batch_norm=batch_norm), nn.ReLU6(False))
        self.avgpool = nn.AvgPool2d(input_size // reduction)
        self.view = View()
        self.fc = nn.Linear(last, num_classes)

    def forward(self, x):
        return self.fc(self.view(self.avgpool(self.conv_last(self.blocks(self.conv1(x))))))


def MobileNetV2_1_0(num_classes=1000, input_size=224):
    return MobileNetV2(num_classes, 1.0, input_size)
