"""ResNet-50-D / ResNet-101-D ("Bag of Tricks for Image Classification with Convolutional Neural Networks", He et al., 2019,
section 4.2) written the "fabu" way of ResNet_fabu.py, from the architecture: Eltwise module for the add, one non-inplace ReLU
module per use, View + AvgPool2d head, modules registered in execution order.

What the D variant changes against ResNet_fabu.py:
  * deep stem: 3x3 stride 2 to 32 channels, 3x3 to 32, 3x3 to 64, each with its own batch norm and ReLU, then MaxPool2d(3, 2, 1);
  * the stride sits on the 3x3 convolution of a bottleneck (as in ResNet_fabu.py already);
  * the shortcut of a downsampling block is AvgPool2d(2, 2) followed by a stride-1 1x1 convolution, so no activation is thrown
    away; stage 1's projection changes the width only and has no pool.
The pool of a shortcut reads ReLU(Eltwise) of the block in front of it: in the integer-simulation model that is a NewAdd sum, the
source resident.enable(avgpool=True, sums=True) serves with fq_avgpool_i16_nhwc.  scripts/resnetd_cost.py measures it on this
model.

`input_size` must be a multiple of 32: the shortcut pools run in floor mode (the published definition; timm's uses
ceil_mode=True, which the integer pool does not take), and on an odd plane a floor-mode 2x2 / 2 pool gives (H - 1) / 2 rows where
the stride-2 3x3 convolution with padding 1 of the main branch gives (H + 1) / 2, so the two operands of the add would disagree.
A multiple of 32 keeps every plane in front of a downsampling block even.

Batch norms are folded by common.quantity.merge_bn before calibration, as for ResNet_fabu.py.
Cared tensors: image + 3 stem conv + 52 conv + 1 fc + 16 Eltwise = 73 (ResNet-50-D).
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Eltwise, View  # noqa: E402


class BottleneckD(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, project=False):
        super(BottleneckD, self).__init__()
        out_planes = planes * self.expansion
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu1 = nn.ReLU(False)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu2 = nn.ReLU(False)
        self.conv3 = nn.Conv2d(planes, out_planes, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_planes)
        shortcut = []
        if project:
            if stride != 1:
                shortcut.append(nn.AvgPool2d(kernel_size=stride, stride=stride))          # floor mode, count_include_pad moot
            shortcut += [nn.Conv2d(inplanes, out_planes, kernel_size=1, stride=1, bias=False), nn.BatchNorm2d(out_planes)]
        self.downsample = nn.Sequential(*shortcut)
        self.Eltwise = Eltwise()
        self.relu3 = nn.ReLU(False)

    def forward(self, x):
        y = self.relu1(self.bn1(self.conv1(x)))
        y = self.relu2(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return self.relu3(self.Eltwise(y, self.downsample(x)))


class ResNetDFabu(nn.Module):

    def __init__(self, layers, num_classes=1000, input_size=224):
        super(ResNetDFabu, self).__init__()
        if input_size < 32 or input_size % 32:
            raise ValueError("ResNet-D: input_size must be a multiple of 32 (floor-mode shortcut pools), got %r" % (input_size,))
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 32, kernel_size=3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(32)
        self.relu1 = nn.ReLU(False)
        self.conv2 = nn.Conv2d(32, 32, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(32)
        self.relu2 = nn.ReLU(False)
        self.conv3 = nn.Conv2d(32, 64, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(64)
        self.relu3 = nn.ReLU(False)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0], 1)
        self.layer2 = self._make_layer(128, layers[1], 2)
        self.layer3 = self._make_layer(256, layers[2], 2)
        self.layer4 = self._make_layer(512, layers[3], 2)
        self.avgpool = nn.AvgPool2d(input_size // 32)
        self.view = View()
        self.fc = nn.Linear(512 * BottleneckD.expansion, num_classes)

    def _make_layer(self, planes, blocks, stride):
        stage = [BottleneckD(self.inplanes, planes, stride, True)]
        self.inplanes = planes * BottleneckD.expansion
        stage += [BottleneckD(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*stage)

    def forward(self, x):
        x = self.relu1(self.bn1(self.conv1(x)))
        x = self.relu2(self.bn2(self.conv2(x)))
        x = self.maxpool(self.relu3(self.bn3(self.conv3(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(self.view(self.avgpool(x)))


def ResNet50D(num_classes=1000, input_size=224):
    return ResNetDFabu([3, 4, 6, 3], num_classes, input_size)


def ResNet101D(num_classes=1000, input_size=224):
    return ResNetDFabu([3, 4, 23, 3], num_classes, input_size)
