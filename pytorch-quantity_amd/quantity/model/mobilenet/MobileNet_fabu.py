"""MobileNetV1-shaped network in "fabu" style: a 3x3 stem (stride 2), thirteen depthwise-separable blocks (depthwise 3x3 -> BN ->
ReLU -> pointwise 1x1 -> BN -> ReLU; widths 32 ... 1024), a global average pool and a Linear classifier.  The flatten and the
residual adds are marker MODULES (View, Eltwise) and every ReLU is out-of-place nn.ReLU, so forward hooks see each cared tensor
and merge_bn -> Quantity -> Reconstruction.ReconModel take the model as it stands.

The reference ships no separable model; this one is written from the architecture (Howard et al. 2017, table 1), in the style
of model/resnet/ResNet_18_fabu.py.  It is the model the depthwise integer kernel (fq_dwconv2d_i8_resident) is measured on
(scripts/depthwise_cost.py).

`residual=True` is a variant that exercises more of the integer path in one file:
  * an identity shortcut (Eltwise) around every stride-1 block whose input and output widths match -- the pointwise layer then
    carries no ReLU of its own, the ReLU follows the add;
  * 5x5 depthwise kernels (padding 2) in the last stage (the two 1024-wide blocks: stride 2 and stride 1).
nn.ReLU only, as the paper has it; the ReLU6 network is model/mobilenetv2/MobileNetV2_fabu.py (the resident plan fuses an nn.ReLU6
with resident.enable(..., relu6=True)).
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Eltwise, View  # noqa: E402

STEM_WIDTH = 32
# (output width, stride of the depthwise layer) of the thirteen blocks
BLOCKS = ((64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1), (512, 1), (512, 1), (512, 1),
          (1024, 2), (1024, 1))
LAST_STAGE_WIDTH = 1024


def _conv_bn(cin, cout, k, stride, pad, groups=1):
    return [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad, groups=groups, bias=False), nn.BatchNorm2d(cout)]


class SeparableBlock(nn.Module):
    """relu(pw(relu(dw(x)))), or with a shortcut relu(Eltwise(pw(relu(dw(x))), x))."""

    def __init__(self, inchannel, outchannel, stride=1, kernel=3, shortcut=False):
        super(SeparableBlock, self).__init__()
        assert not shortcut or (stride == 1 and inchannel == outchannel)
        self.dw = nn.Sequential(*_conv_bn(inchannel, inchannel, kernel, stride, kernel // 2, groups=inchannel), nn.ReLU(False))
        self.pw = nn.Sequential(*_conv_bn(inchannel, outchannel, 1, 1, 0))
        self.Eltwise = Eltwise() if shortcut else None
        self.relu = nn.ReLU(False)

    def forward(self, x):
        y = self.pw(self.dw(x))
        if self.Eltwise is not None:
            y = self.Eltwise(y, x)
        return self.relu(y)


class MobileNet(nn.Module):

    def __init__(self, num_classes=1000, input_size=224, residual=False):
        super(MobileNet, self).__init__()
        assert input_size % 32 == 0, "five stride-2 layers: the input size must be a multiple of 32"
        self.conv1 = nn.Sequential(*_conv_bn(3, STEM_WIDTH, 3, 2, 1), nn.ReLU(False))
        blocks = nn.Sequential()
        width = STEM_WIDTH
        for n, (out, stride) in enumerate(BLOCKS):
            kernel = 5 if (residual and out == LAST_STAGE_WIDTH) else 3
            blocks.add_module(str(n), SeparableBlock(width, out, stride, kernel, shortcut=residual and stride == 1 and width == out))
            width = out
        self.blocks = blocks
        self.avgpool = nn.AvgPool2d(input_size // 32)
        self.view = View()
        self.fc = nn.Linear(width, num_classes)

    def forward(self, x):
        return self.fc(self.view(self.avgpool(self.blocks(self.conv1(x)))))


def MobileNetV1(num_classes=1000, input_size=224):
    return MobileNet(num_classes, input_size, residual=False)


def MobileNetV1Residual(num_classes=1000, input_size=224):
    return MobileNet(num_classes, input_size, residual=True)
