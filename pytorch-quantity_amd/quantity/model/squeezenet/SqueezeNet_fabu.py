"""SqueezeNet-1.1-shaped network in "fabu" style: a 3x3 stride-2 stem, eight Fire modules (squeeze 1x1 -> ReLU -> expand 1x1 +
ReLU and expand 3x3 + ReLU side by side -> Concat), three max-pools, a final 1x1 convolution to the classes with its ReLU, a
global average pool and a View.  The concatenation and the flatten are marker MODULES (Concat, View) and every ReLU is an
out-of-place nn.ReLU of its own, so forward hooks see each cared tensor and Quantity -> Reconstruction.ReconModel take the model
as it stands; the calibrator puts the two expand layers of a Fire module into one merge group (one interval, one bit).

The reference ships no such model; this one is written from the architecture (Iandola et al. 2016; the 1.1 revision's widths),
in the style of model/resnet/ResNet_18_fabu.py.  It is the model the integer Concat kernel (fq_concat_i8_nhwc) is measured on
(scripts/concat_cost.py).  Two deliberate differences from the published network: the max-pools use ceil_mode=False (the
resident plan declines ceil_mode), and there is no Dropout in front of the classifier (not an op the calibrator knows; it is
the identity at inference).  Every expand width is a multiple of 16, so the model runs the kernel's aligned path throughout.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Concat, View  # noqa: E402

STEM_WIDTH = 64
# (squeeze width, width of EACH expand branch) of the eight Fire modules; "pool": a 3x3 stride-2 max-pool
LAYOUT = ("pool", (16, 64), (16, 64), "pool", (32, 128), (32, 128), "pool", (48, 192), (48, 192), (64, 256), (64, 256))


class Fire(nn.Module):
    """Concat(relu(expand1x1(s)), relu(expand3x3(s))) with s = relu(squeeze(x))."""

    def __init__(self, inchannel, squeeze, expand):
        super(Fire, self).__init__()
        self.squeeze = nn.Conv2d(inchannel, squeeze, kernel_size=1)
        self.squeeze_relu = nn.ReLU(False)
        self.expand1x1 = nn.Conv2d(squeeze, expand, kernel_size=1)
        self.expand1x1_relu = nn.ReLU(False)
        self.expand3x3 = nn.Conv2d(squeeze, expand, kernel_size=3, padding=1)
        self.expand3x3_relu = nn.ReLU(False)
        self.Concat = Concat()

    def forward(self, x):
        s = self.squeeze_relu(self.squeeze(x))
        return self.Concat(self.expand1x1_relu(self.expand1x1(s)), self.expand3x3_relu(self.expand3x3(s)))


class SqueezeNet(nn.Module):

    def __init__(self, num_classes=1000, input_size=224):
        super(SqueezeNet, self).__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(3, STEM_WIDTH, kernel_size=3, stride=2), nn.ReLU(False))
        plane = (input_size - 3) // 2 + 1
        features = nn.Sequential()
        width = STEM_WIDTH
        for n, item in enumerate(LAYOUT):
            if item == "pool":
                features.add_module(str(n), nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=False))
                plane = (plane - 3) // 2 + 1
            else:
                features.add_module(str(n), Fire(width, item[0], item[1]))
                width = 2 * item[1]
        assert plane >= 1, "the input is too small for three max-pools behind the stride-2 stem"
        self.features = features
        self.classifier = nn.Sequential(nn.Conv2d(width, num_classes, kernel_size=1), nn.ReLU(False))
        self.avgpool = nn.AvgPool2d(plane)
        self.view = View()

    def forward(self, x):
        return self.view(self.avgpool(self.classifier(self.features(self.conv1(x)))))


def SqueezeNet1_1(num_classes=1000, input_size=224):
    return SqueezeNet(num_classes, input_size)
