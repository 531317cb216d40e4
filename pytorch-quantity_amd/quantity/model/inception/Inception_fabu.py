"""BN-Inception-shaped network in "fabu" style: a 3x3 stride-2 stem, a 3x3 convolution, a max-pool, two stages of two Inception
blocks with a transition (2x2 average pool -> 1x1 convolution) between them, a final 1x1 convolution to the classes with its
ReLU, a global average pool and a View.  A block has four branches -- 1x1; 1x1 -> 3x3; 1x1 -> 3x3 -> 3x3; 3x3 / stride 1 /
padding 1 AVERAGE pool -> 1x1 -- joined by three nested two-operand Concat markers.  The concatenation and the flatten are marker
MODULES (Concat, View) and every layer has an out-of-place nn.ReLU of its own, so forward hooks see each cared tensor and
Quantity -> Reconstruction.ReconModel take the model as it stands; the calibrator puts the operands of a Concat into one merge
group (one interval, one bit), and a convolution behind an average pool reads at the bit of the pool's source.

The reference ships no such model; this one is written from the architecture (Ioffe & Szegedy 2015: the Inception block with an
average-pool branch and the double 3x3 in place of the 5x5), in the style of model/squeezenet/SqueezeNet_fabu.py, much narrower and
shallower than the published network.  It is the model the windowed integer average pool (fq_avgpool_i8_nhwc) is measured on
(scripts/avgpool_cost.py).  Deliberate differences: the batch norms are taken as already folded into the convolutions (what
merge_bn leaves), the max-pool uses ceil_mode=False (the resident plan declines ceil_mode), the stage transition is the DenseNet-
style average pool + 1x1 convolution, and there is no Dropout in front of the classifier.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Concat, View  # noqa: E402

STEM_WIDTH = 32
CONV2_WIDTH = 64
# a block: (1x1, 3x3 reduce, 3x3, double-3x3 reduce, double-3x3, pool projection); "transition": AvgPool2d(2) -> 1x1 to that width
LAYOUT = ((32, 32, 48, 16, 32, 16), (48, 32, 64, 16, 32, 16), ("transition", 192), (64, 48, 96, 24, 48, 32), (96, 64, 128, 32, 64, 32))


def _conv_relu(seq, name, cin, cout, k, padding=0):
    seq.add_module(name, nn.Conv2d(cin, cout, kernel_size=k, padding=padding))
    seq.add_module(name + "_relu", nn.ReLU(False))


class Inception(nn.Module):
    """Concat(Concat(Concat(b1(x), b3(x)), bd(x)), bp(x)): every branch ends in its own ReLU."""

    def __init__(self, inchannel, c1, r3, c3, rd, cd, cp):
        super(Inception, self).__init__()
        self.b1, self.b3, self.bd, self.bp = nn.Sequential(), nn.Sequential(), nn.Sequential(), nn.Sequential()
        _conv_relu(self.b1, "conv", inchannel, c1, 1)
        _conv_relu(self.b3, "reduce", inchannel, r3, 1)
        _conv_relu(self.b3, "conv", r3, c3, 3, 1)
        _conv_relu(self.bd, "reduce", inchannel, rd, 1)
        _conv_relu(self.bd, "conv_a", rd, cd, 3, 1)
        _conv_relu(self.bd, "conv_b", cd, cd, 3, 1)
        self.bp.add_module("pool", nn.AvgPool2d(kernel_size=3, stride=1, padding=1))
        _conv_relu(self.bp, "conv", inchannel, cp, 1)
        self.Concat1, self.Concat2, self.Concat3 = Concat(), Concat(), Concat()
        self.outchannel = c1 + c3 + cd + cp

    def forward(self, x):
        return self.Concat3(self.Concat2(self.Concat1(self.b1(x), self.b3(x)), self.bd(x)), self.bp(x))


class InceptionNet(nn.Module):

    def __init__(self, num_classes=1000, input_size=224):
        super(InceptionNet, self).__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(3, STEM_WIDTH, kernel_size=3, stride=2, padding=1), nn.ReLU(False))
        self.conv2 = nn.Sequential(nn.Conv2d(STEM_WIDTH, CONV2_WIDTH, kernel_size=3, padding=1), nn.ReLU(False))
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=False)
        plane = ((input_size - 1) // 2 + 1 - 3) // 2 + 1
        features = nn.Sequential()
        width = CONV2_WIDTH
        for n, item in enumerate(LAYOUT):
            if item[0] == "transition":
                t = nn.Sequential()
                t.add_module("pool", nn.AvgPool2d(2))
                _conv_relu(t, "conv", width, item[1], 1)
                features.add_module(str(n), t)
                width, plane = item[1], plane // 2
            else:
                block = Inception(width, *item)
                features.add_module(str(n), block)
                width = block.outchannel
        assert plane >= 1, "the input is too small for the max-pool and the transition behind the stride-2 stem"
        self.features = features
        self.classifier = nn.Sequential(nn.Conv2d(width, num_classes, kernel_size=1), nn.ReLU(False))
        self.avgpool = nn.AvgPool2d(plane)
        self.view = View()

    def forward(self, x):
        return self.view(self.avgpool(self.classifier(self.features(self.maxpool(self.conv2(self.conv1(x)))))))


def BNInception(num_classes=1000, input_size=224):
    return InceptionNet(num_classes, input_size)
