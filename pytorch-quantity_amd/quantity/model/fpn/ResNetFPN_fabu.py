"""ResNet-50 with a feature pyramid ("Feature Pyramid Networks for Object Detection", Lin et al., 2017, section 3) written the
"fabu" way of ResNet_fabu.py, from the architecture: Eltwise module for every add, one non-inplace ReLU module per use, View +
AvgPool2d head, modules registered in execution order.

The trunk is ResNet_fabu.py's (its Bottleneck and stage builder).  On top of it, for the stages C3, C4, C5 (strides 8, 16, 32):
  * a 1x1 lateral convolution to 256 channels per level;
  * the top-down pathway  P5 = lateral5(C5),  P4 = Eltwise(lateral4(C4), up(P5)),  P3 = Eltwise(lateral3(C3), up(P4))  with
    nearest upsampling by 2 (nn.UpsamplingNearest2d);
  * a 3x3 output convolution per level, each with its ReLU.
In the integer-simulation model the second step reads a NewAdd sum through the upsampling: the source
resident.enable(concat=True, topdown=True) serves with fq_add_up_resident.  scripts/topdown_cost.py measures it on this model.

The three pyramid levels end in one classifier so that the model has a single output, as the calibration flow expects: each
level is pooled over its whole plane, the three 256-vectors are added (Eltwise) and go through View and one Linear layer.  A
detection head would read the same three tensors.

`input_size` must be a multiple of 32: every stage halves the plane with a stride-2 3x3 convolution with padding 1, which gives
(H + 1) / 2 rows on an odd plane, where upsampling the coarser level by 2 gives an even number -- the two operands of a top-down
add would disagree.

Batch norms are folded by common.quantity.merge_bn before calibration, as for ResNet_fabu.py.
Cared tensors: image + 53 trunk conv + 3 lateral + 3 output conv + 1 fc + 16 trunk Eltwise + 2 top-down + 2 head Eltwise = 81.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Eltwise, View  # noqa: E402
from model.resnet.ResNet_fabu import Bottleneck  # noqa: E402

FPN_CHANNELS = 256


class ResNetFPNFabu(nn.Module):

    def __init__(self, layers, num_classes=1000, input_size=224):
        super(ResNetFPNFabu, self).__init__()
        if input_size < 32 or input_size % 32:
            raise ValueError("ResNet-FPN: input_size must be a multiple of 32 (the top-down adds need even planes), got %r" % (input_size,))
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(False)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0], 1)
        self.layer2 = self._make_layer(128, layers[1], 2)
        self.layer3 = self._make_layer(256, layers[2], 2)
        self.layer4 = self._make_layer(512, layers[3], 2)
        e = Bottleneck.expansion
        self.lateral5 = nn.Conv2d(512 * e, FPN_CHANNELS, kernel_size=1)
        self.lateral4 = nn.Conv2d(256 * e, FPN_CHANNELS, kernel_size=1)
        self.up5 = nn.UpsamplingNearest2d(scale_factor=2)
        self.Eltwise4 = Eltwise()
        self.lateral3 = nn.Conv2d(128 * e, FPN_CHANNELS, kernel_size=1)
        self.up4 = nn.UpsamplingNearest2d(scale_factor=2)
        self.Eltwise3 = Eltwise()
        self.output5 = nn.Conv2d(FPN_CHANNELS, FPN_CHANNELS, kernel_size=3, padding=1)
        self.relu_o5 = nn.ReLU(False)
        self.output4 = nn.Conv2d(FPN_CHANNELS, FPN_CHANNELS, kernel_size=3, padding=1)
        self.relu_o4 = nn.ReLU(False)
        self.output3 = nn.Conv2d(FPN_CHANNELS, FPN_CHANNELS, kernel_size=3, padding=1)
        self.relu_o3 = nn.ReLU(False)
        self.pool5 = nn.AvgPool2d(input_size // 32)
        self.pool4 = nn.AvgPool2d(input_size // 16)
        self.pool3 = nn.AvgPool2d(input_size // 8)
        self.Eltwise_head1 = Eltwise()
        self.Eltwise_head2 = Eltwise()
        self.view = View()
        self.fc = nn.Linear(FPN_CHANNELS, num_classes)

    def _make_layer(self, planes, blocks, stride):
        project = stride != 1 or self.inplanes != planes * Bottleneck.expansion
        stage = [Bottleneck(self.inplanes, planes, stride, project)]
        self.inplanes = planes * Bottleneck.expansion
        stage += [Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*stage)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        c3 = self.layer2(self.layer1(x))
        c4 = self.layer3(c3)
        c5 = self.layer4(c4)
        p5 = self.lateral5(c5)
        p4 = self.Eltwise4(self.lateral4(c4), self.up5(p5))
        p3 = self.Eltwise3(self.lateral3(c3), self.up4(p4))
        o5 = self.relu_o5(self.output5(p5))
        o4 = self.relu_o4(self.output4(p4))
        o3 = self.relu_o3(self.output3(p3))
        y = self.Eltwise_head1(self.pool5(o5), self.pool4(o4))
        y = self.Eltwise_head2(y, self.pool3(o3))
        return self.fc(self.view(y))


def ResNet50FPN(num_classes=1000, input_size=224):
    return ResNetFPNFabu([3, 4, 6, 3], num_classes, input_size)
