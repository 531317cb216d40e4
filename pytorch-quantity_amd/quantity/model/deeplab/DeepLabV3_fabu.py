"""DeepLabV3 on a bottleneck ResNet-50 in "fabu" style (Chen et al. 2017; the backbone of model/resnet/ResNet_fabu.py without its
pooling head).

  backbone   the 7x7/2 stem, the max pool and the four stages of 3 / 4 / 6 / 3 bottlenecks.  Once the running stride has reached
             `output_stride` (16 or 8) a stage that would halve the plane keeps stride 1 instead and multiplies the dilation of
             the DENSE 3x3 of every block behind its first by 2 (the first block still runs at the dilation it inherits, as
             torchvision's replace_stride_with_dilation does): at output stride 16 the last two 3x3s of layer4 at dilation 2;
             at output stride 8 five 3x3s of layer3 at 2, layer4's first at 2 and its last two at 4.  padding = dilation
  ASPP       on layer4's output (32 * width channels): a 1x1 branch and three DENSE atrous 3x3 branches (rate 6 / 12 / 18, at
             output stride 8 12 / 24 / 36, padding = rate -> BN -> ReLU), each to `head_width` channels, joined by nested
             Concats and projected 1x1 back to `head_width` (256)
  head       a 3x3 convolution -> BN -> ReLU -> the 1x1 classifier -> nn.Upsample(bilinear, x output_stride): logits
             [N, num_classes, input_size, input_size]

The image-pooling branch of the paper's ASPP is LEFT OUT, as in model/deeplab/DeepLabV3Plus_fabu.py and for its reasons; the
dropout is left out too (identity at inference).

Every add is an Eltwise marker, every join a Concat marker and every activation out of place, so forward hooks see each cared
tensor and merge_bn -> Quantity -> Reconstruction.ReconModel take the model as it stands.  Its dilated 3x3s are what
Quantity.own_dilated (FQ_OWN_DILATED=1) puts on fq_conv_dil_f32 in the calibration forward.

The reference ships no DeepLab; this one is written from the architecture.  `width` is the first stage's bottleneck width (64: a
ResNet-50; tests build a narrow network -- every multiple of 16 keeps Cin % 16 == 0 in each dilated layer) and scales the head
with it; `input_size` must be a multiple of 32.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Concat, Eltwise  # noqa: E402

BLOCKS = (3, 4, 6, 3)
ASPP_RATES = {16: (6, 12, 18), 8: (12, 24, 36)}


def _conv_bn_relu(cin, cout, k, dilation=1):
    """conv (padding keeps the plane: dilation * (k // 2)) -> BN -> ReLU"""
    return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=k, padding=dilation * (k // 2), dilation=dilation, bias=False),
                         nn.BatchNorm2d(cout), nn.ReLU(False))


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, project=False):
        super(Bottleneck, self).__init__()
        out_planes = planes * self.expansion
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu1 = nn.ReLU(False)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu2 = nn.ReLU(False)
        self.conv3 = nn.Conv2d(planes, out_planes, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_planes)
        if project:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, out_planes, kernel_size=1, stride=stride, bias=False),
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


class DeepLabV3(nn.Module):

    def __init__(self, num_classes=21, output_stride=16, width=64, input_size=224, head_width=None):
        super(DeepLabV3, self).__init__()
        if output_stride not in ASPP_RATES:
            raise ValueError("DeepLabV3: output_stride must be 16 or 8, got %r" % (output_stride,))
        if input_size < 32 or input_size % 32:
            raise ValueError("DeepLabV3: input_size must be a multiple of 32, got %r" % (input_size,))
        if width < 16 or width % 16:
            raise ValueError("DeepLabV3: width must be a multiple of 16, got %r" % (width,))
        head_width = 4 * width if head_width is None else head_width
        self.inplanes, self.reduction, self.dilation = width, 4, 1
        self.conv1 = nn.Conv2d(3, width, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.relu = nn.ReLU(False)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(width, BLOCKS[0], 1, output_stride)
        self.layer2 = self._make_layer(2 * width, BLOCKS[1], 2, output_stride)
        self.layer3 = self._make_layer(4 * width, BLOCKS[2], 2, output_stride)
        self.layer4 = self._make_layer(8 * width, BLOCKS[3], 2, output_stride)
        self.aspp0 = _conv_bn_relu(self.inplanes, head_width, 1)
        self.aspp = nn.ModuleList(_conv_bn_relu(self.inplanes, head_width, 3, r) for r in ASPP_RATES[output_stride])
        self.aspp_cats = nn.ModuleList(Concat() for _ in self.aspp)
        self.aspp_project = _conv_bn_relu((1 + len(self.aspp)) * head_width, head_width, 1)
        self.head = _conv_bn_relu(head_width, head_width, 3)
        self.classifier = nn.Conv2d(head_width, num_classes, kernel_size=1)
        self.up_logits = nn.Upsample(scale_factor=output_stride, mode="bilinear", align_corners=False)

    def _make_layer(self, planes, blocks, stride, output_stride):
        first = self.dilation                                 # the first block runs at the dilation it inherits
        if stride == 2 and self.reduction == output_stride:
            stride, self.dilation = 1, self.dilation * 2      # the stride becomes dilation, from the second block on
        self.reduction *= stride
        project = stride != 1 or self.inplanes != planes * Bottleneck.expansion
        stage = [Bottleneck(self.inplanes, planes, stride, first, project)]
        self.inplanes = planes * Bottleneck.expansion
        stage += [Bottleneck(self.inplanes, planes, 1, self.dilation) for _ in range(1, blocks)]
        return nn.Sequential(*stage)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        y = self.aspp0(x)
        for branch, cat in zip(self.aspp, self.aspp_cats):
            y = cat(y, branch(x))
        return self.up_logits(self.classifier(self.head(self.aspp_project(y))))
