"""A U-Net over a ResNet-18/34 encoder in "fabu" style (the shape of LinkNet / the ResNet-encoder U-Nets of segmentation
libraries): the skips of the decoder are the outputs of the encoder's stages, each the ReLU of a residual SUM.

  stem      conv7x7(3 -> w, stride 2) -> [BN] -> ReLU -> nn.MaxPool2d(3, 2, 1)                                  plane 1/4
  encoder   four stages of BasicBlocks, relu(Eltwise(left(x), shortcut(x))) with left = conv3x3 -> [BN] -> ReLU -> conv3x3 -> [BN]
            and shortcut = identity or a strided 1x1 conv -> [BN]; widths w, 2w, 4w, 8w, the first block of stages 2 to 4 at
            stride 2; `layers` blocks per stage ((2, 2, 2, 2): ResNet-18, (3, 4, 6, 3): ResNet-34)               planes 1/4 .. 1/32
  center    conv3x3(8w -> 8w) -> [BN] -> ReLU                                                                    plane 1/32
  decoder   three times: nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) -> Concat(skip, up) ->
            conv3x3 -> [BN] -> ReLU -> conv3x3 -> [BN] -> ReLU, the skip being the output of stage 3, 2, 1; widths 4w, 2w, w
  head      conv1x1(w -> num_classes), linear: a dense map [N, num_classes, input_size / 4, input_size / 4] (the stem's two
            halvings are not undone)

Residual adds, joins, pools and upsamplings are modules (Eltwise, Concat, nn.MaxPool2d, nn.Upsample) and every ReLU is out of
place, so forward hooks see each cared tensor and merge_bn -> Quantity -> Reconstruction.ReconModel take the model as it stands.
Every Concat here joins the int16 sum of a resident NewAdd with a bilinear upsampling: resident.enable(..., concat=True,
bilinear=True, requant=True) runs it on fq_concat_rq_i8_nhwc; without `requant` each of them leaves the integer domain.

The reference ships no such model; this one is written from the architecture.  `input_size` must be a multiple of 32: five
halvings, and every skip must meet its upsampled partner at the same size.
"""
import sys

import torch.nn as nn

sys.path.insert(0, '../../')
from common.quantity import Concat, Eltwise  # noqa: E402


def _conv_bn(cin, cout, k, stride, pad, batch_norm):
    layers = [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad, bias=not batch_norm)]
    if batch_norm:
        layers.append(nn.BatchNorm2d(cout))
    return layers


class BasicBlock(nn.Module):
    """relu(Eltwise(left(x), shortcut(x)))"""

    def __init__(self, cin, cout, stride, batch_norm):
        super(BasicBlock, self).__init__()
        trunk = _conv_bn(cin, cout, 3, stride, 1, batch_norm)
        trunk.append(nn.ReLU(False))
        trunk.extend(_conv_bn(cout, cout, 3, 1, 1, batch_norm))
        self.left = nn.Sequential(*trunk)
        self.shortcut = nn.Sequential(*(_conv_bn(cin, cout, 1, stride, 0, batch_norm) if stride != 1 or cin != cout else ()))
        self.Eltwise = Eltwise()
        self.relu = nn.ReLU(False)

    def forward(self, x):
        return self.relu(self.Eltwise(self.left(x), self.shortcut(x)))


def _level(cin, c, batch_norm):
    layers = []
    for a, b in ((cin, c), (c, c)):
        layers.extend(_conv_bn(a, b, 3, 1, 1, batch_norm))
        layers.append(nn.ReLU(False))
    return nn.Sequential(*layers)


class ResUNet(nn.Module):

    def __init__(self, num_classes=2, input_size=224, base_width=64, layers=(2, 2, 2, 2), batch_norm=True, in_channels=3):
        super(ResUNet, self).__init__()
        if base_width < 1 or len(layers) != 4 or min(layers) < 1:
            raise ValueError("ResUNet: base_width must be positive and `layers` four positive block counts, got %r and %r"
                             % (base_width, layers))
        if input_size < 32 or input_size % 32:
            raise ValueError("ResUNet: input_size must be a multiple of 32 (five halvings; every skip meets its upsampled partner "
                             "at the same size), got %r" % (input_size,))
        w = base_width
        widths = [w, 2 * w, 4 * w, 8 * w]
        self.stem = nn.Sequential(*_conv_bn(in_channels, w, 7, 2, 3, batch_norm), nn.ReLU(False))
        self.pool = nn.MaxPool2d(3, 2, 1)
        cin = w
        for idx, (c, n) in enumerate(zip(widths, layers), start=1):
            stage = nn.Sequential()
            for b in range(n):
                stage.add_module(str(b), BasicBlock(cin, c, 2 if (b == 0 and idx > 1) else 1, batch_norm))
                cin = c
            setattr(self, "layer%d" % idx, stage)
        self.center = nn.Sequential(*_conv_bn(cin, cin, 3, 1, 1, batch_norm), nn.ReLU(False))
        self.ups = nn.ModuleList(nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) for _ in range(3))
        self.Concats = nn.ModuleList(Concat() for _ in range(3))
        # decoder step j joins the output of stage 3 - j (width widths[2 - j]) with the upsampled tensor (width widths[3 - j])
        self.decs = nn.ModuleList(_level(widths[2 - j] + widths[3 - j], widths[2 - j], batch_norm) for j in range(3))
        self.head = nn.Conv2d(w, num_classes, kernel_size=1)

    def forward(self, x):
        x = self.pool(self.stem(x))
        skips = []
        for idx in range(1, 5):
            x = getattr(self, "layer%d" % idx)(x)
            skips.append(x)
        x = self.center(skips.pop())
        for up, cat, dec in zip(self.ups, self.Concats, self.decs):
            x = dec(cat(skips.pop(), up(x)))
        return self.head(x)
