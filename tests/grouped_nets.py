"""ResNeXt-style toy nets for the grouped-convolution tests (test infrastructure, no product code), and a table of FIXED bits
for them that follows the dataflow -- depthwise_nets.fixed_info chains the bits in registration order, which a block with a
shortcut does not have.

  fixed_info(model)   {layer name: info}: the input bit of a layer is the output bit of the layer named in the net's SOURCES
                      (default: the layer registered before it; "image": the image bit), so that consecutive integer layers
                      hand integers to each other; weight bits as depthwise_nets.fixed_info gives them, per channel for the
                      grouped / depthwise layers only with per_channel="grouped"; out_bit_of: the output bits, where measured.
Module-level classes, so the rebuilt models pickle.  rebuild / seeded / shifts are depthwise_nets' own.
"""
from collections import OrderedDict

import numpy as np
from torch import nn

from depthwise_nets import rebuild, seeded, shifts  # noqa: F401
from per_channel_chain import numpy_channel_bits


def fixed_info(model, per_channel=False, image_bit=5, seed=0, out_bits=(3, 4, 5), out_bit_of=None, sources=None):
    rng = np.random.default_rng(seed)
    sources = getattr(model, "SOURCES", {}) if sources is None else sources
    info = OrderedDict()
    prev = "image"
    out_bit = {"image": image_bit}
    for name, m in model.named_modules():
        kind = type(m).__name__
        if kind not in ("Conv2d", "Linear"):
            continue
        ib = out_bit[sources.get(name, prev)]
        ob = int(rng.choice(out_bits)) if out_bit_of is None else int(out_bit_of[name])
        wb0, tensor_bit = numpy_channel_bits(m.weight.detach().cpu().numpy())
        cap = 12 - ib + ob
        listed = per_channel is True or (per_channel == "grouped" and kind == "Conv2d" and m.groups > 1)
        wb = [min(b, cap) for b in wb0] if listed else min(tensor_bit, cap)
        info[name] = {"weight_bit": wb, "bias_bit": ob, "input_bit": ib, "output_bit": ob, "layer": m, "layer_type": kind}
        out_bit[name] = ob
        prev = name
    return info


def bottleneck_sources(model):
    """SOURCES of a ResNet / ResNeXt written the fabu way (model/resnext/ResNeXt_fabu.py): a block's conv1 and projection read
    what the block before it produced, whose bit is taken to be that block's conv3's."""
    sources, prev = {}, "conv1"
    for stage in ("layer1", "layer2", "layer3", "layer4"):
        for i, _block in enumerate(getattr(model, stage)):
            base = "%s.%d." % (stage, i)
            sources[base + "conv1"] = prev
            sources[base + "downsample.0"] = prev
            prev = base + "conv3"
    sources["fc"] = prev
    return sources


class XBlock(nn.Module):
    """1x1 -> ReLU -> grouped 3x3 -> ReLU -> 1x1 -> Eltwise with the shortcut -> ReLU."""

    def __init__(self, inplanes, width, out_planes, groups, stride=1):
        from common.quantity import Eltwise
        super(XBlock, self).__init__()
        self.conv1 = nn.Conv2d(inplanes, width, 1)
        self.relu1 = nn.ReLU(False)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, groups=groups)
        self.relu2 = nn.ReLU(False)
        self.conv3 = nn.Conv2d(width, out_planes, 1)
        if stride != 1 or inplanes != out_planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, out_planes, 1, stride=stride))
        else:
            self.downsample = nn.Sequential()
        self.Eltwise = Eltwise()
        self.relu3 = nn.ReLU(False)

    def forward(self, x):
        y = self.relu1(self.conv1(x))
        y = self.relu2(self.conv2(y))
        return self.relu3(self.Eltwise(self.conv3(y), self.downsample(x)))


class ToyResNeXt(nn.Module):
    """Two blocks, 24 -> 32 channels, G = 4: 4 and 8 channels per group, the second block stride 2 with a projection."""
    SOURCES = {"b1.conv1": "stem", "b2.conv1": "b1.conv3", "b2.downsample.0": "b1.conv3", "fc": "b2.conv3"}
    GROUPED = ("b1.conv2", "b2.conv2")

    def __init__(self):
        from common.quantity import View
        super(ToyResNeXt, self).__init__()
        self.stem = nn.Conv2d(3, 24, 3, padding=1)
        self.r0 = nn.ReLU(False)
        self.b1 = XBlock(24, 16, 24, 4)
        self.b2 = XBlock(24, 32, 32, 4, stride=2)
        self.pool = nn.AvgPool2d(4)
        self.view = View()
        self.fc = nn.Linear(32, 5)

    def forward(self, x):
        x = self.b2(self.b1(self.r0(self.stem(x))))
        return self.fc(self.view(self.pool(x)))


class GroupedPointwiseNet(nn.Module):
    """A grouped 1x1 (the pointwise layer of a ShuffleNet unit) between dense layers, and a stride-2 one."""
    GROUPED = ("gp1", "gp2")

    def __init__(self):
        from common.quantity import View
        super(GroupedPointwiseNet, self).__init__()
        self.stem = nn.Conv2d(3, 24, 3, padding=1)
        self.r0 = nn.ReLU(False)
        self.gp1 = nn.Conv2d(24, 48, 1, groups=2)
        self.r1 = nn.ReLU(False)
        self.mid = nn.Conv2d(48, 40, 3, padding=1)
        self.r2 = nn.ReLU(False)
        self.gp2 = nn.Conv2d(40, 20, 1, stride=2, groups=5)
        self.r3 = nn.ReLU(False)
        self.pool = nn.AvgPool2d(4)
        self.view = View()
        self.fc = nn.Linear(20, 5)

    def forward(self, x):
        x = self.r1(self.gp1(self.r0(self.stem(x))))
        x = self.r3(self.gp2(self.r2(self.mid(x))))
        return self.fc(self.view(self.pool(x)))


class GroupedDepthwiseNet(nn.Module):
    """A grouped 3x3 and a depthwise 3x3 in one chain: enable(depthwise=True, grouped=True) takes both."""
    GROUPED = ("gc",)
    DEPTHWISE = ("dw",)

    def __init__(self):
        from common.quantity import View
        super(GroupedDepthwiseNet, self).__init__()
        self.stem = nn.Conv2d(3, 32, 3, padding=1)
        self.r0 = nn.ReLU(False)
        self.gc = nn.Conv2d(32, 32, 3, padding=1, groups=4)
        self.r1 = nn.ReLU(False)
        self.dw = nn.Conv2d(32, 32, 3, stride=2, padding=1, groups=32)
        self.r2 = nn.ReLU(False)
        self.pw = nn.Conv2d(32, 24, 1)
        self.r3 = nn.ReLU(False)
        self.pool = nn.AvgPool2d(4)
        self.view = View()
        self.fc = nn.Linear(24, 5)

    def forward(self, x):
        x = self.r1(self.gc(self.r0(self.stem(x))))
        x = self.r3(self.pw(self.r2(self.dw(x))))
        return self.fc(self.view(self.pool(x)))


class GroupedAddNet(nn.Module):
    """A grouped layer whose output feeds an Eltwise DIRECTLY (no ReLU, no 1x1 between), and one that reads the sum."""
    SOURCES = {"gb": "ga"}
    GROUPED = ("ga", "gb")

    def __init__(self):
        from common.quantity import Eltwise, View
        super(GroupedAddNet, self).__init__()
        self.stem = nn.Conv2d(3, 24, 3, padding=1)
        self.r0 = nn.ReLU(False)
        self.ga = nn.Conv2d(24, 24, 3, padding=1, groups=3)
        self.Eltwise = Eltwise()
        self.r1 = nn.ReLU(False)
        self.gb = nn.Conv2d(24, 48, 3, stride=2, padding=1, groups=6)
        self.r2 = nn.ReLU(False)
        self.pw = nn.Conv2d(48, 24, 1)
        self.r3 = nn.ReLU(False)
        self.pool = nn.AvgPool2d(4)
        self.view = View()
        self.fc = nn.Linear(24, 5)

    def forward(self, x):
        x = self.r0(self.stem(x))
        x = self.r1(self.Eltwise(self.ga(x), x))
        x = self.r3(self.pw(self.r2(self.gb(x))))
        return self.fc(self.view(self.pool(x)))


class TwiceNet(nn.Module):
    """One grouped layer called twice: the plan leaves it alone."""

    def __init__(self):
        from common.quantity import View
        super(TwiceNet, self).__init__()
        self.stem = nn.Conv2d(3, 16, 3, padding=1)
        self.r0 = nn.ReLU(False)
        self.gc = nn.Conv2d(16, 16, 3, padding=1, groups=2)
        self.r1 = nn.ReLU(False)
        self.r2 = nn.ReLU(False)
        self.pw = nn.Conv2d(16, 16, 1)
        self.r3 = nn.ReLU(False)
        self.pool = nn.AvgPool2d(8)
        self.view = View()
        self.fc = nn.Linear(16, 5)

    def forward(self, x):
        x = self.r1(self.gc(self.r0(self.stem(x))))
        x = self.r2(self.gc(x))
        return self.fc(self.view(self.pool(self.r3(self.pw(x)))))


def g16_net():
    """The net of golden G16 (tests/golden/make_golden_grouped.py): ToyResNeXt, seeded by cases.seed_model."""
    return ToyResNeXt()


G16_SHAPE = (4, 3, 8, 8)
G16_SEED, G16_CALIB_SEED, G16_INPUT_SEED = 16, 1600, 1616
