"""ShuffleNetV2 in "fabu" style: a 3x3 stem (stride 2) to 24 channels -> BN -> ReLU, a 3x3 stride-2 max-pool, three stages of
(4, 8, 4) units, a 1x1 conv5 -> BN -> ReLU, a global average pool and a Linear classifier.

  stride-1 unit   the input is split into two halves by the marker modules Slice(0, c/2) and Slice(c/2, c); the right half goes
                  through 1x1 -> BN -> ReLU -> depthwise 3x3 -> BN -> 1x1 -> BN -> ReLU; Concat(left, right); nn.ChannelShuffle(2).
  stride-2 unit   (the first of a stage) two branches on the whole input -- depthwise 3x3 stride 2 -> BN -> 1x1 -> BN -> ReLU, and
                  1x1 -> BN -> ReLU -> depthwise 3x3 stride 2 -> BN -> 1x1 -> BN -> ReLU --, then Concat and the shuffle.

The split, the join and the shuffle are modules (Slice, Concat, nn.ChannelShuffle), the flatten is the marker module View and
every activation is an out-of-place nn.ReLU(False), so forward hooks see each cared tensor and merge_bn -> Quantity ->
Reconstruction.ReconModel take the model as it stands (tools/configs.yml lists ChannelShuffle and Slice among the traced op
types).  Every convolution is a dense 1x1, a depthwise 3x3 or the stem: resident.enable(..., depthwise=True, concat=True,
shuffle=True) keeps the whole network between the stem and conv5 in int8.

The reference ships no ShuffleNet; this one is written from the architecture (Ma et al. 2018, table 5), in the style of
model/mobilenetv2/MobileNetV2_fabu.py.  `width_mult` picks a column of the table (0.5, 1.0, 1.5, 2.0); `stages` (repeats per
stage) and `widths` (the three stage widths and conv5's) replace it (tests build a small network with them; stage widths must be
even); `input_size` must be a multiple of the network's reduction (32 with three stages); `batch_norm=False` builds the network as merge_bn leaves it (convolutions with a
bias, no BatchNorm), which is what tests with hand-made integer weights want.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Concat, Slice, View  # noqa: E402

STEM_WIDTH = 24
STAGES = (4, 8, 4)
# multiplier -> (stage 2, stage 3, stage 4, conv5): table 5 of the paper
WIDTHS = {0.5: (48, 96, 192, 1024), 1.0: (116, 232, 464, 1024), 1.5: (176, 352, 704, 1024), 2.0: (244, 488, 976, 2048)}


def _conv_bn(cin, cout, k, stride, pad, groups=1, batch_norm=True):
    if not batch_norm:
        return [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad, groups=groups, bias=True)]
    return [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad, groups=groups, bias=False), nn.BatchNorm2d(cout)]


def _pw_relu(cin, cout, batch_norm):
    return nn.Sequential(*_conv_bn(cin, cout, 1, 1, 0, batch_norm=batch_norm), nn.ReLU(False))


def _dw(c, stride, batch_norm):
    return nn.Sequential(*_conv_bn(c, c, 3, stride, 1, groups=c, batch_norm=batch_norm))


class ShuffleUnit(nn.Module):
    """stride 1: shuffle(Concat(x[:, :c/2], branch(x[:, c/2:]))); stride 2: shuffle(Concat(down(x), branch(x)))."""

    def __init__(self, inchannel, outchannel, stride, batch_norm=True):
        super(ShuffleUnit, self).__init__()
        assert stride in (1, 2) and outchannel % 2 == 0
        half = outchannel // 2
        if stride == 1:
            assert inchannel == outchannel
            self.left = Slice(0, half)
            self.right = Slice(half, inchannel)
            self.down = None
            cin = half
        else:
            self.left = self.right = None
            self.down = nn.Sequential(_dw(inchannel, 2, batch_norm), _pw_relu(inchannel, half, batch_norm))
            cin = inchannel
        self.branch = nn.Sequential(_pw_relu(cin, half, batch_norm), _dw(half, stride, batch_norm), _pw_relu(half, half, batch_norm))
        self.Concat = Concat()
        self.shuffle = nn.ChannelShuffle(2)

    def forward(self, x):
        if self.down is None:
            y = self.Concat(self.left(x), self.branch(self.right(x)))
        else:
            y = self.Concat(self.down(x), self.branch(x))
        return self.shuffle(y)


class ShuffleNetV2(nn.Module):

    def __init__(self, num_classes=1000, width_mult=1.0, input_size=224, stages=STAGES, widths=None, batch_norm=True):
        super(ShuffleNetV2, self).__init__()
        widths = tuple(WIDTHS[width_mult] if widths is None else widths)
        assert len(widths) == len(stages) + 1, "one width per stage and one for conv5"
        width = STEM_WIDTH
        self.conv1 = nn.Sequential(*_conv_bn(3, width, 3, 2, 1, batch_norm=batch_norm), nn.ReLU(False))
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        units = nn.Sequential()
        reduction = 4
        for repeats, out in zip(stages, widths[:-1]):
            for i in range(repeats):
                units.add_module(str(len(units)), ShuffleUnit(width, out, 2 if i == 0 else 1, batch_norm))
                width = out
            reduction *= 2
        self.units = units
        assert input_size % reduction == 0, "the input size must be a multiple of the stride-2 layers' product, %d" % reduction
        self.conv5 = _pw_relu(width, widths[-1], batch_norm)
        self.avgpool = nn.AvgPool2d(input_size // reduction)
        self.view = View()
        self.fc = nn.Linear(widths[-1], num_classes)

    def forward(self, x):
        return self.fc(self.view(self.avgpool(self.conv5(self.units(self.maxpool(self.conv1(x)))))))


def ShuffleNetV2_1_0(num_classes=1000, input_size=224):
    return ShuffleNetV2(num_classes, 1.0, input_size)
