"""Shared by the tests of the resident add with a nearest-upsampled operand (test infrastructure, no product code): the kernel's
case list and sources, small integer-simulation nets with an FPN top-down pathway built directly from NewConv2d info dicts -- no
calibration, so the CPU suite (on the doubles of tests/topdown_doubles.py) and the GPU suite build the same nets --, the float toy
of golden G24 and the random family RandomTopDown.  Module-level classes, so a planned net pickles.

Bits: an image at bit 5, activations at bit 4 unless a test says otherwise; the sum of two operands at bits gx, gy lies on the grid
g = max(0, gx, gy).
"""
import random

import numpy as np
import torch
from torch import nn

from concat_nets import conv, example  # noqa: F401  (re-exported for the tests)


def pad16(c):
    return (c + 15) // 16 * 16


# ---------------------------------------------------------------- the kernel's cases
# (N, H, W, C, up): H, W the OUTPUT plane.  2x2 only at up = 2; 4x12: a row of three coarse pixels; 8x8: more than one coarse row
PLANES = ((2, 2), (4, 4), (4, 12), (8, 8))
KERNEL_CASES = [(n, h, w, c, up) for up in (2, 4) for n in (1, 3) for (h, w) in PLANES for c in (1, 16, 19, 100)
                if h % up == 0 and w % up == 0]
# csrc/fq_add_up_geom.h: a launch has at most kAddUpMaxBlocks = 4096 workgroups of kAddUpBlock = 256 lanes, one item (16 channels
# of a pixel) per lane and round.  At 48 channels (3 items per pixel, so the digit-wise walk carries) the smallest square plane with
# more items than lanes is 592 x 592: 592 * 592 * 3 = 1 051 392 > 1 048 576 >= 590 * 590 * 3
LANES = 4096 * 256
SECOND_ITEM_CASE = (1, 592, 592, 48, 2)
GRIDS = (-2, 0, 3, 8)
K_VALUES = (-2, 0, 1, 8, 9)                                  # g - ib: <= 0 and 9 the int32 form, 1 and 8 the packed one


def case_arg(case):
    return "%d,%d,%d,%d,%d" % tuple(case)


def source(rng, shape, c, dtype, g):
    """An int8 / int16 NHWC operand on grid g whose padding channels hold non-zero garbage: int8 over its whole range, int16 over
    what an exact sum on grid g holds, [-128 * 2^g, 127 * 2^g] (g < 0: the int8 range), both ends planted."""
    if dtype == np.int8:
        lo, hi = -128, 127
    else:
        lo, hi = (-128 << max(g, 0)), (127 << max(g, 0))
    a = rng.integers(lo, hi + 1, size=shape).astype(dtype)
    a.flat[::7] = lo
    a.flat[3::11] = hi
    a[..., c:] = np.where(a[..., c:] == 0, 77, a[..., c:])
    return a


def repeat(y, up):
    """Nearest upsampling of an NHWC array: what the kernel never writes."""
    return np.repeat(np.repeat(y, up, axis=1), up, axis=2)


# ---------------------------------------------------------------- a top-down pathway of two steps
class TopDownNet(nn.Module):
    """stem + ReLU (16 x 16) -> d1 + ReLU (8 x 8) -> d2 + ReLU (4 x 4); lateral 1x1 convolutions l2, l3, l4; the pathway
        p4 = l4(c4);  s3 = add1(l3(c3), up1(p4));  s2 = add2(l2(c2), up2(s3))
    and a 3x3 output convolution per level (o4, o3, o2; the model's three outputs).  up1 reads an int8 activation, up2 the sum s3,
    which o3 reads as well.  What a test varies:
    up          step (1, 2) -> its upsampling module (default nn.UpsamplingNearest2d(scale_factor=factor))
    bits        output bits of (l4, l3, l2): s3 lies on max(0, l4, l3), s2 on max(0, that, l2)
    read_bits   input bits of (o3, o2)
    relu_sum    a ReLU behind each add (the add fuses it; the upsampling then reads ReLU(sum))
    swap        the upsampled operand comes first
    factor      4: d1 and d2 have stride 4 and the image is 32 x 32 (planes 32, 8, 2)
    mode        "plain"; "relu_behind": a ReLU between up2 and add2; "twice": one module is up1 and up2; "extra_reader": a 1x1
                convolution reads up2's value besides add2; "extra_reader_int8": the same behind up1; "both_up": add1's other
                operand is upsampled too (from a second 4 x 4 lateral); "foreign_lateral": add2's other operand is fp32 code."""

    def __init__(self, up=None, bits=(4, 4, 4), read_bits=(4, 4), relu_sum=False, swap=False, factor=2, mode="plain"):
        from common.quantity import NewAdd
        super(TopDownNet, self).__init__()
        make_up = (lambda step: nn.UpsamplingNearest2d(scale_factor=factor)) if up is None else up
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.d1, self.r1 = conv(16, 16, 3, 4, 4, stride=factor, padding=1, seed=1), nn.ReLU()
        self.d2, self.r2 = conv(16, 16, 3, 4, 4, stride=factor, padding=1, seed=2), nn.ReLU()
        self.l4, self.l3, self.l2 = (conv(16, 16, 1, 4, bits[0], seed=3), conv(16, 16, 1, 4, bits[1], seed=4),
                                     conv(16, 16, 1, 4, bits[2], seed=5))
        self.up1 = make_up(1)
        self.up2 = self.up1 if mode == "twice" else make_up(2)
        self.add1, self.add2 = NewAdd(), NewAdd()
        self.ra1, self.ra2 = nn.ReLU(), nn.ReLU()
        self.o4 = conv(16, 8, 3, bits[0], 4, padding=1, seed=6)
        self.o3, self.o2 = conv(16, 8, 3, read_bits[0], 4, padding=1, seed=7), conv(16, 8, 3, read_bits[1], 4, padding=1, seed=8)
        if mode == "relu_behind":
            self.rup = nn.ReLU()
        if mode in ("extra_reader", "extra_reader_int8"):
            self.side = conv(16, 8, 1, 4, 4, seed=9)
        if mode == "both_up":
            self.l4b, self.up1b = conv(16, 16, 1, 4, bits[1], seed=10), make_up(1)
        self.relu_sum, self.swap, self.mode, self.factor = relu_sum, swap, mode, factor

    def example(self, n=4, seed=1):
        return example(n, 16 if self.factor == 2 else 32, seed)

    def _add(self, add, lateral, top):
        return add(top, lateral) if self.swap else add(lateral, top)

    def forward(self, x):
        c2 = self.r0(self.stem(x))
        c3 = self.r1(self.d1(c2))
        c4 = self.r2(self.d2(c3))
        p4 = self.l4(c4)
        extra = []
        u1 = self.up1(p4)
        if self.mode == "extra_reader_int8":
            extra.append(self.side(u1))
        s3 = self._add(self.add1, self.up1b(self.l4b(c4)) if self.mode == "both_up" else self.l3(c3), u1)
        if self.relu_sum:
            s3 = self.ra1(s3)
        u2 = self.up2(s3)
        if self.mode == "relu_behind":
            u2 = self.rup(u2)
        if self.mode == "extra_reader":
            extra.append(self.side(u2))
        lat2 = self.l2(c2)
        if self.mode == "foreign_lateral":
            lat2 = lat2 * 1.0
        s2 = self._add(self.add2, lat2, u2)
        if self.relu_sum:
            s2 = self.ra2(s2)
        return (self.o2(s2), self.o3(s3), self.o4(p4)) + tuple(extra)


# ---------------------------------------------------------------- golden G24
class G24Net(nn.Module):
    """The FLOAT net calibrated for golden G24 (tests/golden/make_golden_topdown.py): a toy FPN on 3 x 16 x 16 input -- a trunk of
    three stages (16, 8 and 4 pixels wide), 1x1 laterals, two nearest-x2 top-down steps with Eltwise, a 3x3 output convolution on
    the middle sum -- which the second upsampling reads as well -- and on the last one, whose result goes through a global pool,
    View and Linear: one tensor out.  The marker layers come from whichever `common.quantity` is imported: the reference's when
    the golden is captured, the product's in the tests."""

    def __init__(self):
        from common.quantity import Eltwise, View
        super(G24Net, self).__init__()
        self.stem, self.relu0 = nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(False)
        self.down1, self.relu1 = nn.Conv2d(8, 16, 3, stride=2, padding=1), nn.ReLU(False)
        self.down2, self.relu2 = nn.Conv2d(16, 16, 3, stride=2, padding=1), nn.ReLU(False)
        self.lat4, self.lat3, self.lat2 = nn.Conv2d(16, 8, 1), nn.Conv2d(16, 8, 1), nn.Conv2d(8, 8, 1)
        self.up1, self.up2 = nn.UpsamplingNearest2d(scale_factor=2), nn.UpsamplingNearest2d(scale_factor=2)
        self.Eltwise1, self.Eltwise2 = Eltwise(), Eltwise()
        self.out3, self.relu3 = nn.Conv2d(8, 8, 3, stride=2, padding=1), nn.ReLU(False)
        self.out2, self.relu4 = nn.Conv2d(8, 8, 3, stride=4, padding=1), nn.ReLU(False)
        self.Eltwise3 = Eltwise()
        self.pool_g = nn.AvgPool2d(4)
        self.view = View()
        self.fc = nn.Linear(8, 5)

    def forward(self, x):
        c2 = self.relu0(self.stem(x))
        c3 = self.relu1(self.down1(c2))
        c4 = self.relu2(self.down2(c3))
        s3 = self.Eltwise1(self.lat3(c3), self.up1(self.lat4(c4)))
        s2 = self.Eltwise2(self.lat2(c2), self.up2(s3))
        y = self.Eltwise3(self.relu3(self.out3(s3)), self.relu4(self.out2(s2)))
        return self.fc(self.view(self.pool_g(y)))


def g24_net():
    return G24Net()


G24_SHAPE = (4, 3, 16, 16)
G24_SEED, G24_CALIB_SEED, G24_INPUT_SEED = 24, 2400, 2424


# ---------------------------------------------------------------- the random family
class RandomTopDown(nn.Module):
    """A random FPN-shaped integer-simulation net drawn from `seed`: finest plane 8 or 16, batch 4, widths 8 to 64, 2 or 3 levels
    below the finest, every step down and up by a factor of 2 or 4 (whichever the plane allows), lateral output bits 2 .. 6, an
    optional fused ReLU behind a sum, the upsampled operand first or second.  Every level has a 3x3 output convolution (the
    model's outputs).  One upsampling in six is made one the rule declines: a second reader (a 1x1 convolution) or a ReLU behind
    it.  `ups`: [(module name, admitted, reads a sum)]."""

    def __init__(self, seed):
        from common.quantity import NewAdd
        super(RandomTopDown, self).__init__()
        rng = random.Random(seed)
        self.plane = rng.choice((8, 16))
        width = rng.choice((8, 16, 24, 64))
        self.stem, self.r0 = conv(3, width, 3, 5, 4, padding=1, seed=seed), nn.ReLU()
        levels, plane, factors = rng.choice((2, 3)), self.plane, []
        for _ in range(levels):
            ok = [f for f in (2, 4) if plane % f == 0 and plane // f >= 1]
            if not ok:
                break
            factors.append(rng.choice(ok))
            plane //= factors[-1]
        self.factors = factors
        downs, relus, lats, outs, ups, adds, radds, sides = [], [], [], [], [], [], [], {}
        fw = rng.choice((8, 16, 32))                         # the pathway's width
        for i, f in enumerate(factors):
            downs.append(conv(width, width, 3, 4, 4, stride=f, padding=1, seed=seed + i))
            relus.append(nn.ReLU())
        for i in range(len(factors) + 1):                    # lateral i reads level i (0: the finest)
            lats.append(conv(width, fw, 1, 4, rng.randint(2, 6), seed=seed + 10 + i))
        self.ups, self.relu_sum, self.swap, self.decline = [], [], [], {}
        for j in range(len(factors)):                        # step j goes from level n - j to level n - j - 1
            f = factors[len(factors) - 1 - j]
            ups.append(nn.UpsamplingNearest2d(scale_factor=f) if rng.random() < 0.5 else nn.Upsample(scale_factor=f, mode="nearest"))
            adds.append(NewAdd())
            radds.append(nn.ReLU())
            self.relu_sum.append(rng.random() < 0.5)
            self.swap.append(rng.random() < 0.5)
            admitted = True
            if rng.random() < 1.0 / 6:
                kind = rng.choice(("reader", "relu"))
                self.decline[j] = kind
                if kind == "reader":
                    sides[str(j)] = conv(fw, 8, 1, 4, 4, seed=seed + 30 + j)
                else:
                    sides[str(j)] = nn.ReLU()
                admitted = False
            # a declined upsampling over a SUM has the fp32 form only, so the add behind it is not resident and the next
            # upsampling finds no integer source: not admitted either.  (Declined over int8 it keeps its int8 launch.)
            if j > 0 and not integer_sum:
                admitted = False
            integer_sum = admitted or j == 0
            self.ups.append(("ups.%d" % j, admitted, j > 0))
        for i in range(len(factors) + 1):
            outs.append(conv(fw, 8, 3, rng.randint(2, 6), 4, padding=1, seed=seed + 20 + i))
        self.downs, self.relus, self.lats, self.outs = nn.ModuleList(downs), nn.ModuleList(relus), nn.ModuleList(lats), nn.ModuleList(outs)
        self.up_mods, self.adds, self.radds, self.sides = nn.ModuleList(ups), nn.ModuleList(adds), nn.ModuleList(radds), nn.ModuleDict(sides)
        # (the names in `ups` are those of up_mods)
        self.ups = [("up_mods.%d" % j, ok, over) for j, (_n, ok, over) in enumerate(self.ups)]

    def example(self, seed=1):
        return torch.randn(4, 3, self.plane, self.plane, generator=torch.Generator().manual_seed(seed))

    def forward(self, x):
        feats = [self.r0(self.stem(x))]
        for d, r in zip(self.downs, self.relus):
            feats.append(r(d(feats[-1])))
        n = len(self.factors)
        top = self.lats[n](feats[n])
        outs, extra = [self.outs[n](top)], []
        for j in range(n):
            level = n - 1 - j
            u = self.up_mods[j](top)
            kind = self.decline.get(j)
            if kind == "reader":
                extra.append(self.sides[str(j)](u))
            elif kind == "relu":
                u = self.sides[str(j)](u)
            lat = self.lats[level](feats[level])
            top = self.adds[j](u, lat) if self.swap[j] else self.adds[j](lat, u)
            if self.relu_sum[j]:
                top = self.radds[j](top)
            outs.append(self.outs[level](top))
        return tuple(outs) + tuple(extra)
