"""ImageNet-style ResNeXt (aggregated residual transformations: the bottleneck's 3x3 is a grouped convolution of
`cardinality` groups, `base_width` channels per group in the first stage, doubling per stage) written with marker layers in
the manner of ResNet_fabu.py, so that the calibrator sees every residual add.

Written from the architecture: Eltwise module for the add, one non-inplace ReLU module per use, View + AvgPool2d head, and
modules registered in execution order (the table writer pairs named_modules() order with execution order).  It goes through
merge_bn -> Quantity -> Reconstruction.ReconModel unchanged.

ResNeXt-50 32x4d: the 3x3 layers have 32 groups of 4 / 8 / 16 / 32 input and output channels per group (widths 128 / 256 /
512 / 1024) -- sixteen grouped layers, the ones fq_gconv2d_i8_resident serves under resident.enable(..., grouped=True).
Cared tensors: image + 53 conv + 1 fc + 16 Eltwise = 71, as ResNet-50.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Eltwise, View  # noqa: E402


class XBottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, cardinality, base_width, stride=1, project=False):
        super(XBottleneck, self).__init__()
        width = int(planes * base_width / 64.0) * cardinality
        out_planes = planes * self.expansion
        self.conv1 = nn.Conv2d(inplanes, width, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.relu1 = nn.ReLU(False)
        self.conv2 = nn.Conv2d(width, width, kernel_size=3, stride=stride, padding=1, groups=cardinality, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.relu2 = nn.ReLU(False)
        self.conv3 = nn.Conv2d(width, out_planes, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_planes)
        if project:
            self.downsample = nn.Sequential(
                nn.Conv2d(inplanes, out_planes, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(out_planes))
        else:
            self.downsample = nn.Sequential()
        self.Eltwise = Eltwise()
        self.relu3 = nn.ReLU(False)

    def forward(self, x):
        y = self.relu1(self.bn1(self.conv1(x)))
        y = self.relu2(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return self.relu3(self.Eltwise(y, self.downsample(x)))


class ResNeXtFabu(nn.Module):

    def __init__(self, layers, cardinality=32, base_width=4, num_classes=1000, input_size=224):
        super(ResNeXtFabu, self).__init__()
        self.cardinality = cardinality
        self.base_width = base_width
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(False)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0], 1)
        self.layer2 = self._make_layer(128, layers[1], 2)
        self.layer3 = self._make_layer(256, layers[2], 2)
        self.layer4 = self._make_layer(512, layers[3], 2)
        self.avgpool = nn.AvgPool2d(max(input_size // 32, 1))
        self.view = View()
        self.fc = nn.Linear(512 * XBottleneck.expansion, num_classes)

    def _make_layer(self, planes, blocks, stride):
        project = stride != 1 or self.inplanes != planes * XBottleneck.expansion
        stage = [XBottleneck(self.inplanes, planes, self.cardinality, self.base_width, stride, project)]
        self.inplanes = planes * XBottleneck.expansion
        stage += [XBottleneck(self.inplanes, planes, self.cardinality, self.base_width) for _ in range(1, blocks)]
        return nn.Sequential(*stage)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(self.view(self.avgpool(x)))


def ResNeXt50(num_classes=1000, input_size=224, cardinality=32, base_width=4):
    return ResNeXtFabu([3, 4, 6, 3], cardinality, base_width, num_classes, input_size)


def ResNeXt101(num_classes=1000, input_size=224, cardinality=32, base_width=8):
    return ResNeXtFabu([3, 4, 23, 3], cardinality, base_width, num_classes, input_size)
