"""The nets and case lists of the bilinear-upsampling tests (test infrastructure, no product code).

  KERNEL_PLANES / KERNEL_CHANNELS / KERNEL_SHIFTS   the cases of tests/test_gpu_upsample_bilinear_i8.py;
                       scripts/upsample_bilinear_geom_check.cpp walks the same planes and channel counts.
  DecoderNet(variant)  a two-level U-Net-shaped integer-simulation net built from NewConv2d info dicts (no calibration): what
                       enable(concat=True, bilinear=True) plans.  DECODER_VARIANTS names the variants.
  DeclinedNet(variant) one small net per reason for which a bilinear upsampling stays torch's.  DECLINED maps the variant to a
                       piece of its describe().bilinear_left text.
  g25_net()            golden G25: the FLOAT net calibrated by tests/golden/make_golden_bilinear.py.  Imports under the REFERENCE's
                       `common` package too: Concat / View come from whichever `common.quantity` is imported.
  RandomBilinearNet(seed)   the random family: a U-Net-shaped net with 1 to 3 decoder levels, factors 2 and 4, bits 2 .. 6.
  unet_model(**kw)     model/unet/UNet_fabu.py's UNet.
"""
import random

import torch
from torch import nn

import common.quantity as _cq
from shuffle_nets import Slice

Concat, View = _cq.Concat, _cq.View

KERNEL_PLANES = ((1, 1), (1, 5), (3, 2), (2, 3), (7, 9), (8, 8))
BIG_PLANE = (33, 47)                       # more than one workgroup at every channel count below
KERNEL_CHANNELS = (1, 16, 19, 33, 80)
KERNEL_SHIFTS = (-8, -3, -1, 0, 2, 5, 8)
CLOSED_FORM_GRIDS = (-2, 0, 3, 8)
CLOSED_FORM_PLANES = ((1, 1), (1, 5), (3, 2), (7, 9), (8, 8))


def bilinear(factor=2, **kw):
    return nn.Upsample(scale_factor=factor, mode="bilinear", align_corners=False, **kw)


def example(n=4, size=16, seed=1):
    return torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------- what is planned
DECODER_VARIANTS = ("plain", "relu", "x4", "conv", "pool", "slice", "shift")


class DecoderNet(nn.Module):
    """stem + ReLU (16 ch, full plane) -> pool -> enc + ReLU (24 ch, 1/2) -> pool -> bott + ReLU (32 ch, 1/4) -> mid (1x1, 24 ch,
    linear: negative values are interpolated) -> up1 -> Concat(skip, up1) -> dec1 + ReLU -> up2 -> Concat(skip, up2) -> dec2 + ReLU
    -> head.  By `variant`:
      "plain"   as above, both factors 2               "relu"    an nn.ReLU directly behind up1 (the kernel's flag)
      "x4"      one level: up1 by 4 from 1/4 to the full plane, joined with the stem's skip
      "conv"    up1 straight into dec1 (no Concat)      "pool"    up1 -> MaxPool2d(3, 1, 1) -> Concat
      "slice"   up1 -> Slice(4, 20) -> Concat           "shift"   mid writes on grid 2, dec1 reads at bit 4: shift 2
    `ups`: the names of the bilinear modules; `front`: the convolutions in front of them."""

    def __init__(self, variant="plain"):
        from concat_nets import conv
        super(DecoderNet, self).__init__()
        assert variant in DECODER_VARIANTS
        self.variant = v = variant
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.pool1 = nn.MaxPool2d(2)
        self.enc, self.r1 = conv(16, 24, 3, 4, 4, padding=1), nn.ReLU()
        self.pool2 = nn.MaxPool2d(2)
        self.bott, self.r2 = conv(24, 32, 3, 4, 4, padding=1), nn.ReLU()
        self.mid = conv(32, 24, 1, 4, 2 if v == "shift" else 4)
        self.up1 = bilinear(4 if v == "x4" else 2)
        if v == "relu":
            self.r_up = nn.ReLU()
        if v == "pool":
            self.mp = nn.MaxPool2d(3, 1, 1)
        if v == "slice":
            self.cut = Slice(4, 20)
        if v != "conv":
            self.cat1 = Concat()
        skip1 = {"x4": 16, "conv": 0}.get(v, 24)
        self.dec1, self.r3 = conv(skip1 + (16 if v == "slice" else 24), 16, 3, 4, 4, padding=1, seed=3), nn.ReLU()
        self.ups, self.front = ["up1"], ["mid"]
        if v != "x4":
            self.up2, self.cat2 = bilinear(2), Concat()
            self.dec2, self.r4 = conv(32, 8, 3, 4, 4, padding=1, seed=4), nn.ReLU()
            self.ups.append("up2")
            self.front.append("dec1")
        self.head = conv(16 if v == "x4" else 8, 4, 1, 4, 4, seed=5)

    def forward(self, x):
        v = self.variant
        e1 = self.r0(self.stem(x))
        e2 = self.r1(self.enc(self.pool1(e1)))
        u = self.up1(self.mid(self.r2(self.bott(self.pool2(e2)))))
        if v == "relu":
            u = self.r_up(u)
        if v == "pool":
            u = self.mp(u)
        if v == "slice":
            u = self.cut(u)
        if v == "x4":
            return self.head(self.r3(self.dec1(self.cat1(e1, u))))
        d1 = self.r3(self.dec1(u if v == "conv" else self.cat1(e2, u)))
        return self.head(self.r4(self.dec2(self.cat2(e1, self.up2(d1)))))


# ---------------------------------------------------------------- what is declined
DECLINED = {
    "align_corners": "align_corners=True", "size": "`size=` form", "factor3": "scale_factor 3", "factor1.5": "scale_factor 1.5",
    "two_factors": "scale_factor (2.0, 4.0)", "twice": "more than once", "sum": "NewAdd sum (int16)", "lossy": "lossy value of act",
    "no_source": "no integer source", "fp32_source": "no integer form", "two_bits": "different bits [3, 4]",
    "add": "read as fp32 by the NewAdd add",
    "avgpool": "read as fp32 by the average pool avg", "act": "read as fp32 by the table activation act2", "output": "model output",
    "foreign": "code outside the plan", "shift": "|b - g| = |7 - -2| > 8",
}


class DeclinedNet(nn.Module):
    """A 3 -> 16 stem + ReLU at bit 4, a 1x1 `mid` (16 ch, output grid 4) and the bilinear upsampling `up` behind it, read by the
    1x1 `head` at bit 4 -- planned as it stands ("ok") -- and by `variant` one thing that makes the plan leave `up` to torch (the
    keys of DECLINED).  Module-level, so the planned net pickles."""

    def __init__(self, variant):
        from concat_nets import conv
        from common.quantity import NewAdd
        super(DeclinedNet, self).__init__()
        assert variant == "ok" or variant in DECLINED
        self.variant = v = variant
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.mid = conv(16, 16, 1, 4, -2 if v == "shift" else 4)
        self.up = {"align_corners": lambda: nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True),
                   "size": lambda: nn.Upsample(size=(16, 16), mode="bilinear", align_corners=False),
                   "factor3": lambda: bilinear(3), "factor1.5": lambda: bilinear(1.5),
                   "two_factors": lambda: bilinear((2, 4))}.get(v, bilinear)()
        if v == "sum":
            self.other, self.pre = conv(16, 16, 1, 4, 4, seed=2), NewAdd()
        if v in ("lossy", "act"):
            self.act = nn.Hardswish()
        if v == "act":
            self.act2 = nn.Hardswish()
        if v == "add":
            self.big, self.add = conv(3, 16, 1, 5, 4, seed=3), NewAdd()
        if v == "avgpool":
            self.avg = nn.AvgPool2d(3, 1, 1)
        if v == "fp32_source":
            self.ceil = nn.MaxPool2d(3, 1, 1, ceil_mode=True)
        if v == "two_bits":
            self.side = conv(16, 8, 1, 3, 4, seed=7)
        self.head = conv(32 if v == "foreign" else 16, 8, 1, 7 if v == "shift" else 4, 4, seed=9)

    def forward(self, x):
        v = self.variant
        s = self.r0(self.stem(x))
        m = self.mid(s)
        if v == "sum":
            m = self.pre(m, self.other(s))
        if v == "lossy":
            m = self.act(m)
        if v == "no_source":
            m = m * 1.0                                       # (foreign code: the upsampling's input is no traced value)
        if v == "fp32_source":
            m = self.ceil(m)                                  # (a ceil_mode max-pool is traced but not planned: its value is fp32)
        u = self.up(m)
        if v == "twice":
            return self.head(self.up(u)[:, :, ::2, ::2].contiguous())
        if v == "add":
            return self.head(self.add(u, self.big(torch.cat((x, x), 2).repeat(1, 1, 1, 2))))
        if v == "avgpool":
            return self.head(self.avg(u))
        if v == "act":
            return self.head(self.act2(u))
        if v == "output":
            return self.head(u), u
        if v == "foreign":
            return self.head(torch.cat((u, u), 1))
        if v == "two_bits":
            return self.head(u), self.side(u)
        return self.head(u)


# ---------------------------------------------------------------- golden G25
G25_SHAPE = (4, 3, 16, 16)
G25_SEED, G25_CALIB_SEED, G25_INPUT_SEED = 18, 2500, 2525     # (the weight seed: one whose calibrated Concats sit on their readers' bits)
G25_UPS = ("up1", "up2", "up3")


class G25Net(nn.Module):
    """The FLOAT net calibrated for golden G25: an encoder of three levels (16, 8 and 4 pixels), a linear 1x1, two decoder levels
    -- bilinear x2 (an nn.ReLU directly behind the first) -> Concat(skip, up) -> conv + ReLU --, then MaxPool2d(4) -> 1x1 ->
    bilinear x4 straight into a stride-4 convolution, a global pool, View and a Linear: one tensor out."""

    def __init__(self):
        super(G25Net, self).__init__()
        self.conv1, self.relu1 = nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(False)
        self.pool1 = nn.MaxPool2d(2)
        self.conv2, self.relu2 = nn.Conv2d(8, 12, 3, 1, 1), nn.ReLU(False)
        self.pool2 = nn.MaxPool2d(2)
        self.conv3, self.relu3 = nn.Conv2d(12, 16, 3, 1, 1), nn.ReLU(False)
        self.conv4 = nn.Conv2d(16, 12, 1)
        self.up1, self.relu_up, self.Concat1 = bilinear(2), nn.ReLU(False), Concat()
        self.conv5, self.relu5 = nn.Conv2d(24, 8, 3, 1, 1), nn.ReLU(False)
        self.up2, self.Concat2 = bilinear(2), Concat()
        self.conv6, self.relu6 = nn.Conv2d(16, 8, 3, 1, 1), nn.ReLU(False)
        self.pool3 = nn.MaxPool2d(4)
        self.conv7 = nn.Conv2d(8, 8, 1)
        self.up3 = bilinear(4)
        self.conv8, self.relu8 = nn.Conv2d(8, 8, 3, 4, 1), nn.ReLU(False)
        self.avgpool, self.view, self.fc = nn.AvgPool2d(4), View(), nn.Linear(8, 5)

    def forward(self, x):
        e1 = self.relu1(self.conv1(x))
        e2 = self.relu2(self.conv2(self.pool1(e1)))
        b = self.conv4(self.relu3(self.conv3(self.pool2(e2))))
        d1 = self.relu5(self.conv5(self.Concat1(e2, self.relu_up(self.up1(b)))))
        d2 = self.relu6(self.conv6(self.Concat2(e1, self.up2(d1))))
        y = self.relu8(self.conv8(self.up3(self.conv7(self.pool3(d2)))))
        return self.fc(self.view(self.avgpool(y)))


def g25_net():
    return G25Net()


# ---------------------------------------------------------------- the random family
class RandomBilinearNet(nn.Module):
    """A random U-Net-shaped integer-simulation net drawn from `seed`: finest plane 8 or 16, batch 4, widths 8 to 64, 1 to 3
    decoder levels, every step down and up by a factor of 2 or 4 (whichever the plane allows), bits 2 .. 6.  Going down: a 3x3
    convolution + ReLU and a MaxPool2d(factor) per level.  At the bottom a 1x1 convolution (linear, or with a ReLU), then per
    decoder step: bilinear upsampling (now and then with an nn.ReLU directly behind it) -> Concat with the level's skip, or straight
    into the convolution -> 3x3 convolution + ReLU.  The skip of a level is written at the bit the step's convolution reads, and
    the convolution in front of an upsampling on a grid of its own (shift = bit - grid in [-4, 4]).  One upsampling in five is
    made one the rule declines: a second reader at another bit, a NewAdd reader, align_corners=True, or a factor given as
    `size=`.  `ups`: [(module name, admitted)]; `factors`: the factors drawn."""

    DECLINES = ("two_bits", "add", "align_corners", "size")

    def __init__(self, seed):
        from concat_nets import conv
        from common.quantity import NewAdd
        super(RandomBilinearNet, self).__init__()
        rng = random.Random(1000 + seed)
        self.plane = rng.choice((8, 16))
        levels, plane, factors = rng.choice((1, 2, 3)), self.plane, []
        for _ in range(levels):
            ok = [f for f in (2, 4) if plane % f == 0 and plane // f >= 1]
            if not ok:
                break
            factors.append(rng.choice(ok))
            plane //= factors[-1]
        self.factors = factors
        n = len(factors)
        widths = [rng.choice((8, 12, 16, 24, 32, 64)) for _ in range(n + 1)]
        read = [rng.randint(2, 6) for _ in range(n)]         # read[i]: the bit at which decoder convolution of level i reads
        encs, relus, pools = [], [], []
        cin, ib = 3, 5
        for i in range(n + 1):
            ob = read[i] if i < n else rng.randint(2, 6)     # (the skip of level i is written at the bit its reader reads)
            encs.append(conv(cin, widths[i], 3, ib, ob, padding=1, seed=seed + i))
            relus.append(nn.ReLU())
            if i < n:
                pools.append(nn.MaxPool2d(factors[i]))
            cin, ib = widths[i], ob
        self.encs, self.relus, self.pools = nn.ModuleList(encs), nn.ModuleList(relus), nn.ModuleList(pools)
        fronts, ups, cats, decs, drelus, extras = [], [], [], [], [], {}
        self.front_relu, self.relu_up, self.join, self.decline, self.ups = [], [], [], {}, []
        for j in range(n):                                   # step j goes from level n - j to level n - j - 1
            level = n - 1 - j
            f = factors[level]
            b = read[level]
            g = min(6, max(-1, b + rng.randint(-4, 4)))
            c = rng.choice((8, 16, 20, 24))
            fronts.append(conv(cin, c, 1, ib, g, seed=seed + 10 + j))
            self.front_relu.append(rng.random() < 0.3)
            self.relu_up.append(rng.random() < 0.25)
            self.join.append(rng.random() < 0.75)
            up, admitted = bilinear(f), True
            if rng.random() < 0.2:
                kind = rng.choice(self.DECLINES)
                self.decline[j] = kind
                admitted = False
                if kind == "two_bits":
                    extras["side%d" % j] = conv(c, 8, 1, b + 1, 4, seed=seed + 30 + j)
                elif kind == "add":
                    extras["add%d" % j] = NewAdd()
                elif kind == "align_corners":
                    up = nn.Upsample(scale_factor=f, mode="bilinear", align_corners=True)
                else:
                    size = self.plane
                    for lf in factors[:level]:
                        size //= lf
                    up = nn.Upsample(size=(size, size), mode="bilinear", align_corners=False)
            ups.append(up)
            extras["r_up%d" % j], extras["r_front%d" % j] = nn.ReLU(), nn.ReLU()
            cats.append(Concat())
            ob = rng.randint(2, 6)
            decs.append(conv(c + (widths[level] if self.join[j] else 0), widths[level], 3, b, ob, padding=1, seed=seed + 20 + j))
            drelus.append(nn.ReLU())
            cin, ib = widths[level], ob
            self.ups.append(("up_mods.%d" % j, admitted))
        self.fronts, self.up_mods, self.cats, self.decs, self.drelus = (nn.ModuleList(fronts), nn.ModuleList(ups), nn.ModuleList(cats),
                                                                          nn.ModuleList(decs), nn.ModuleList(drelus))
        self.extras = nn.ModuleDict(extras)
        self.head = conv(cin, 4, 1, ib, 4, seed=seed + 40)

    def example(self, seed=1):
        return torch.randn(4, 3, self.plane, self.plane, generator=torch.Generator().manual_seed(seed))

    def forward(self, x):
        skips, outs = [], []
        n = len(self.factors)
        for i in range(n + 1):
            x = self.relus[i](self.encs[i](x))
            if i < n:
                skips.append(x)
                x = self.pools[i](x)
        for j in range(n):
            t = self.fronts[j](x)
            if self.front_relu[j]:
                t = self.extras["r_front%d" % j](t)
            u = self.up_mods[j](t)
            kind = self.decline.get(j)
            if kind == "two_bits":
                outs.append(self.extras["side%d" % j](u))
            elif kind == "add":
                u = self.extras["add%d" % j](u, u)
            if self.relu_up[j]:
                u = self.extras["r_up%d" % j](u)
            skip = skips.pop()
            x = self.drelus[j](self.decs[j](self.cats[j](skip, u) if self.join[j] else u))
        return (self.head(x),) + tuple(outs)


SEEDS = list(range(40))


def unet_model(**kw):
    """model/unet/UNet_fabu.py's UNet (the product's `common` package must be the imported one)."""
    import importlib.util
    import os
    import sys
    name = "_fq_unet_fabu"
    mod = sys.modules.get(name)
    if mod is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-quantity_amd", "quantity", "model",
                            "unet", "UNet_fabu.py")
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return mod.UNet(**kw)
