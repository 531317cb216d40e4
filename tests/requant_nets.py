"""The nets and case lists of the re-quantising-Concat tests (test infrastructure, no product code).

  kernel_cases() / sources() / case_arg()   the cases of tests/test_gpu_concat_rq_i8.py; scripts/concat_geom_check.cpp walks the
                       same shapes.
  ToyNet(variant)      one small integer-simulation net per cause for which the plain rule does not serve a Concat and
                       enable(concat=True, requant=True) does; built from NewConv2d info dicts, no calibration.
  DeclinedNet(variant) one small net per reason for which the re-quantising rule declines.  DECLINED maps the variant to a piece of
                       its describe().requant_left text.
  g26_net()            golden G26: the FLOAT net calibrated by tests/golden/make_golden_requant.py.  Imports under the REFERENCE's
                       `common` package too: Concat / Eltwise / View come from whichever `common.quantity` is imported.
  RandomRequantNet(seed)   the random family.
  resunet_model(**kw)  model/unet/ResUNet_fabu.py's ResUNet.
"""
import itertools
import random

import numpy as np
import torch
from torch import nn

import common.quantity as _cq

Concat, Eltwise, View = _cq.Concat, _cq.Eltwise, _cq.View


def pad16(c):
    return (int(c) + 15) // 16 * 16


def bilinear(factor=2):
    return nn.Upsample(scale_factor=factor, mode="bilinear", align_corners=False)


def example(n=4, size=8, seed=1):
    return torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------- the kernel's cases
KERNEL_N = (1, 3)
KERNEL_PLANES = ((1, 1), (2, 2), (4, 12), (8, 8))
KERNEL_NSRC = (1, 2, 3, 8)
KERNEL_CHANNELS = (1, 3, 16, 19, 33, 100)
KERNEL_UPS = (1, 2, 4)
KERNEL_SHIFTS = (-8, -3, -1, 0, 1, 8)
BIG_CASE = (3, 120, 120, (100, 100), (1, 2), (2, 1), (-3, 1), (0, 1))      # 561 600 chunks: past 2048 x 256 lanes


def _channel_lists(nsrc):
    ch = KERNEL_CHANNELS
    if nsrc == 1:
        return [(c,) for c in ch]
    if nsrc == 2:
        return [(16, 16), (1, 3), (19, 33), (100, 16), (3, 100), (33, 19), (16, 1)]
    if nsrc == 3:
        return [(16, 16, 16), (1, 3, 16), (19, 33, 100), (100, 1, 3), (33, 16, 19)]
    return [(16,) * 8, (1, 3, 16, 19, 33, 100, 1, 3), (100, 33, 19, 16, 3, 1, 16, 16)]


def _byte_mixes(nsrc):
    if nsrc <= 3:
        return list(itertools.product((1, 2), repeat=nsrc))                # every int8 / int16 mix
    return [(1,) * 8, (2,) * 8, (1, 2) * 4, (2, 1) * 4, (2, 2, 1, 1, 2, 1, 1, 2)]


def kernel_cases(nsrc, plane):
    """[(N, H, W, Cs, ups, bytes, shifts, relus)] for one source count and one output plane: every channel list of the count with
    every element-size mix, the factors, shifts and ReLU flags cycled through so that each value meets each source position."""
    H, W = plane
    out, tick = [], 0
    ups_ok = [u for u in KERNEL_UPS if H % u == 0 and W % u == 0]
    for N in KERNEL_N:
        for Cs in _channel_lists(nsrc):
            for by in _byte_mixes(nsrc):
                ups = tuple(ups_ok[(tick + i) % len(ups_ok)] for i in range(nsrc))
                shifts = tuple(KERNEL_SHIFTS[(tick + 2 * i) % len(KERNEL_SHIFTS)] for i in range(nsrc))
                relus = tuple((tick >> i) & 1 for i in range(nsrc)) if nsrc <= 3 else tuple((tick + i) % 3 == 0 for i in range(nsrc))
                relus = tuple(int(r) for r in relus)
                if nsrc == 1 and by[0] == 1 and ups[0] == 1 and not relus[0] and shifts[0] == 0:
                    shifts = (1,)                                            # (the call with nothing to do is an argument error)
                out.append((N, H, W, tuple(Cs), ups, tuple(by), shifts, relus))
                tick += 1
    return out


def case_arg(case):
    """The case as scripts/concat_geom_check.cpp reads it: N,H,W/C.../up.../bytes..."""
    N, H, W, Cs, ups, by = case[:6]
    return "%d,%d,%d/%s/%s/%s" % (N, H, W, ",".join(map(str, Cs)), ",".join(map(str, ups)), ",".join(map(str, by)))


def sources(rng, case):
    """One array per source, [N, H / up, W / up, pad16(C)] of int8 or int16: random over the whole range of the type -- the padding
    channels too: garbage the kernel must not let through --, with the extremes (+-127 / -128, -32768, 32767) and, for a negative
    shift, exact ties (odd multiples of 2^(-shift - 1), with even and with odd quotients) planted among the real channels."""
    N, H, W, Cs, ups, by, shifts, _relus = case
    arrays = []
    for C, up, b, shift in zip(Cs, ups, by, shifts):
        dt, lo, hi = (np.int8, -128, 127) if b == 1 else (np.int16, -32768, 32767)
        a = rng.integers(lo, hi + 1, (N, H // up, W // up, pad16(C))).astype(dt)
        real = a[..., :C].reshape(-1)
        plant = [lo, hi, -127, 127, -128, 0, 1, -1]
        if shift < 0:
            half = 1 << (-shift - 1)
            plant += [v for j in (-5, -4, -3, -2, -1, 0, 1, 2, 3, 4) for v in ((2 * j + 1) * half,) if lo <= v <= hi]
        at = rng.permutation(real.size)[:len(plant)]
        real[at] = np.array(plant[:at.size], dtype=dt)
        a[..., :C] = real.reshape(a[..., :C].shape)
        arrays.append(a)
    return arrays


def model_launches():
    """The launch shapes of the two models of scripts/requant_concat_cost.py as walker cases: UNet(base_width 32, depth 4) and
    ResUNet at its defaults, 224 x 224, one image (the walker's cost is per pixel; the batch only repeats the plane)."""
    unet = [(1, 224 >> (3 - j), 224 >> (3 - j), (32 << (3 - j), 32 << (3 - j)), (1, 1), (1, 1), (0, 0), (0, 0)) for j in range(4)]
    res = [(1, 7 << (j + 1), 7 << (j + 1), (256 >> j, 512 >> j), (1, 1), (2, 1), (0, 0), (0, 0)) for j in range(3)]
    return unet + res


# ---------------------------------------------------------------- what is planned
TOY_VARIANTS = ("reader_bit", "two_grids", "sum", "sum_relu", "upsampled", "bilinear")


class ToyNet(nn.Module):
    """stem (3 -> 16, 3x3) + ReLU at bit 4, then by `variant` one Concat `cat` that the plain rule does not serve:
      "reader_bit"  a (16 ch) and b (24 ch) both on grid 4, a ReLU behind the Concat, the head reads at bit 3
      "two_grids"   a (20 ch) on grid 4, b (12 ch) on grid 2, the head reads at bit 4 (a chunk holds bytes of both)
      "sum"         Eltwise(a, b) -- grids 4 and 3, the sum on grid 4 -- joined with c (8 ch, grid 5); no ReLU: negative values
      "sum_relu"    ReLU(Eltwise(a, b)) joined with c; a second convolution reads the sum's int8 form at bit 4 as well
      "upsampled"   coarse (16 ch, grid 2, half the plane) -> nearest x2 -> Concat with fine (24 ch, grid 4), a ReLU behind it
      "bilinear"    mid (24 ch, grid 4, half the plane) -> bilinear x2 -> Concat(skip on grid 3, up), the decoder reads at bit 4:
                    the parent's plan revokes the upsampling (bilinear_nets' test), this one plans both
    `fronts`: the producers that go from emit_f32 to integers only (in front of the Concat; "reader_bit": the Concat itself, which
    the plain rule plans and makes emit fp32; "upsampled": the nearest upsampling, which is folded into the launch); `kw`: further enable() arguments of
    both arms; `launch`: [(channels, bytes, up, relu, shift)] of the Concat's one launch."""

    def __init__(self, variant):
        from concat_nets import conv
        from common.quantity import NewAdd
        super(ToyNet, self).__init__()
        assert variant in TOY_VARIANTS
        self.variant = v = variant
        self.kw = {}
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.cat = Concat()
        if v == "reader_bit":
            self.a, self.b = conv(16, 16, 1, 4, 4), conv(16, 24, 3, 4, 4, padding=1)
            self.r1 = nn.ReLU()
            self.head = conv(40, 8, 1, 3, 4, seed=5)
            self.fronts, self.launch = ("cat",), [(16, 1, 1, True, -1), (24, 1, 1, True, -1)]
        elif v == "two_grids":
            self.a, self.b = conv(16, 20, 1, 4, 4), conv(16, 12, 3, 4, 2, padding=1)
            self.head = conv(32, 8, 1, 4, 4, seed=5)
            self.fronts, self.launch = ("a", "b"), [(20, 1, 1, False, 0), (12, 1, 1, False, 2)]
        elif v in ("sum", "sum_relu"):
            self.a, self.b = conv(16, 16, 1, 4, 4), conv(16, 16, 3, 4, 3, padding=1)
            self.add = NewAdd()
            self.c = conv(16, 8, 1, 4, 5, seed=2)
            if v == "sum_relu":
                self.r1 = nn.ReLU()
                self.side = conv(16, 8, 1, 4, 4, seed=7)
            self.head = conv(24, 8, 1, 4, 4, seed=5)
            self.fronts, self.launch = ("add", "c"), [(16, 2, 1, False, 0), (8, 1, 1, False, -1)]
        elif v == "upsampled":
            self.fine = conv(16, 24, 3, 4, 4, padding=1)
            self.down, self.r1 = conv(16, 32, 3, 4, 4, stride=2, padding=1), nn.ReLU()
            self.coarse = conv(32, 16, 1, 4, 2)
            self.up = nn.UpsamplingNearest2d(scale_factor=2)
            self.r2 = nn.ReLU()
            self.head = conv(40, 8, 1, 4, 4, seed=5)
            self.fronts, self.launch = ("up", "fine"), [(16, 1, 2, True, 2), (24, 1, 1, True, 0)]
        else:
            self.kw = dict(bilinear=True)
            self.skip, self.r1 = conv(16, 24, 3, 4, 3, padding=1), nn.ReLU()
            self.pool = nn.MaxPool2d(2)
            self.mid = conv(24, 24, 1, 3, 4)
            self.up = bilinear(2)
            self.head, self.r2 = conv(48, 8, 3, 4, 4, padding=1, seed=5), nn.ReLU()
            self.fronts, self.launch = ("skip", "mid"), [(24, 1, 1, False, 1), (24, 1, 1, False, 0)]

    def forward(self, x):
        v = self.variant
        s = self.r0(self.stem(x))
        if v == "reader_bit":
            return self.head(self.r1(self.cat(self.a(s), self.b(s))))
        if v == "two_grids":
            return self.head(self.cat(self.a(s), self.b(s)))
        if v == "sum":
            return self.head(self.cat(self.add(self.a(s), self.b(s)), self.c(s)))
        if v == "sum_relu":
            t = self.r1(self.add(self.a(s), self.b(s)))
            return self.head(self.cat(t, self.c(s))), self.side(t)
        if v == "upsampled":
            u = self.up(self.coarse(self.r1(self.down(s))))
            return self.head(self.r2(self.cat(u, self.fine(s))))
        e = self.r1(self.skip(s))
        return self.r2(self.head(self.cat(e, self.up(self.mid(self.pool(e))))))


# ---------------------------------------------------------------- what is declined
DECLINED = {
    "two_bits": "different bits [3, 4]", "output": "model output", "add": "read as fp32 by the NewAdd add2",
    "up_sum": "upsampled NewAdd sum", "shift": "|b - g| = |7 - -2| > 8", "twice": "more than once", "dim": "dim != 1",
    "no_source": "not the output of a planned layer", "fp32_source": "no integer form",
}


class DeclinedNet(nn.Module):
    """A 3 -> 16 stem + ReLU at bit 4, a (16 ch, grid 4) and b (16 ch, grid 2) joined by `cat` and read by the 1x1 `head` at bit 4
    -- planned as it stands ("ok") -- and by `variant` one thing that makes the re-quantising rule decline (the keys of DECLINED).
    Module-level, so the planned net pickles."""

    def __init__(self, variant):
        from concat_nets import conv
        from common.quantity import NewAdd
        super(DeclinedNet, self).__init__()
        assert variant == "ok" or variant in DECLINED
        self.variant = v = variant
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        g = -2 if v == "shift" else 4
        self.a, self.b = conv(16, 16, 1, 4, g), conv(16, 16, 3, 4, g if v == "shift" else 2, padding=1)
        self.cat = Concat()
        if v == "two_bits":
            self.side = conv(32, 8, 1, 3, 4, seed=7)
        if v == "add":
            self.c, self.add2 = conv(16, 32, 1, 4, 4, seed=3), NewAdd()
        if v == "up_sum":
            self.pool = nn.MaxPool2d(2)
            self.b2 = conv(16, 16, 3, 4, 3, padding=1, seed=4)
            self.add, self.up = NewAdd(), nn.UpsamplingNearest2d(scale_factor=2)
        if v == "fp32_source":
            self.ceil = nn.MaxPool2d(3, 1, 1, ceil_mode=True)
        hb = 7 if v == "shift" else 4
        self.head = conv(16 if v == "dim" else 32, 8, 1, hb, 4, seed=9)

    def forward(self, x):
        v = self.variant
        s = self.r0(self.stem(x))
        a, b = (None, None) if v == "up_sum" else (self.a(s), self.b(s))
        if v == "no_source":
            b = b * 1.0                                       # (foreign code: the operand is no traced value)
        if v == "fp32_source":
            b = self.ceil(b)                                  # (a ceil_mode max-pool is traced but not planned: its value is fp32)
        if v == "up_sum":                                     # (a and b2 on the pooled plane, their sum upsampled; b on the full one)
            p = self.pool(s)
            a, b = self.up(self.add(self.a(p), self.b2(p))), self.b(s)
        if v == "dim":
            return self.head(self.cat(a, b, 2)[:, :, ::2].contiguous())
        c = self.cat(a, b)
        if v == "twice":
            return self.head(self.cat(c[:, :16].contiguous(), c[:, 16:].contiguous()))
        if v == "two_bits":
            return self.head(c), self.side(c)
        if v == "output":
            return self.head(c), c
        if v == "add":
            return self.head(self.add2(c, self.c(s)))
        return self.head(c)


# ---------------------------------------------------------------- golden G26
G26_SHAPE = (4, 3, 16, 16)
G26_SEED, G26_CALIB_SEED, G26_INPUT_SEED = 3, 2600, 2626       # (the weight seed: the first of 0 .. 3 whose calibration meets the maker's conditions)


class G26Net(nn.Module):
    """The FLOAT net calibrated for golden G26: conv1 + ReLU (16 px), a pool, a residual block on 8 px -- conv2 + ReLU -> conv3,
    Eltwise(conv3, pool1), ReLU: the SKIP --, a pool, conv4 + ReLU (4 px), conv5 (1x1, linear), bilinear x2 -> Concat1(skip, up) ->
    conv6 + ReLU; then two branches conv7 (1x1) and conv8 (3x3) of conv6's output -> Concat2 -> ReLU -> conv9 + ReLU, a global pool,
    View and a Linear: one tensor out."""

    def __init__(self):
        super(G26Net, self).__init__()
        self.conv1, self.relu1 = nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(False)
        self.pool1 = nn.MaxPool2d(2)
        self.conv2, self.relu2 = nn.Conv2d(8, 8, 3, 1, 1), nn.ReLU(False)
        self.conv3 = nn.Conv2d(8, 8, 3, 1, 1)
        self.Eltwise1, self.relu3 = Eltwise(), nn.ReLU(False)
        self.pool2 = nn.MaxPool2d(2)
        self.conv4, self.relu4 = nn.Conv2d(8, 16, 3, 1, 1), nn.ReLU(False)
        self.conv5 = nn.Conv2d(16, 8, 1)
        self.up1, self.Concat1 = bilinear(2), Concat()
        self.conv6, self.relu6 = nn.Conv2d(16, 8, 3, 1, 1), nn.ReLU(False)
        self.conv7 = nn.Conv2d(8, 8, 1)
        self.conv8 = nn.Conv2d(8, 8, 3, 1, 1)
        self.Concat2, self.relu_cat = Concat(), nn.ReLU(False)
        self.conv9, self.relu9 = nn.Conv2d(16, 8, 3, 1, 1), nn.ReLU(False)
        self.avgpool, self.view, self.fc = nn.AvgPool2d(8), View(), nn.Linear(8, 5)

    def forward(self, x):
        p = self.pool1(self.relu1(self.conv1(x)))
        skip = self.relu3(self.Eltwise1(self.conv3(self.relu2(self.conv2(p))), p))
        b = self.conv5(self.relu4(self.conv4(self.pool2(skip))))
        d = self.relu6(self.conv6(self.Concat1(skip, self.up1(b))))
        y = self.relu9(self.conv9(self.relu_cat(self.Concat2(self.conv7(d), self.conv8(d)))))
        return self.fc(self.view(self.avgpool(y)))


def g26_net():
    return G26Net()


# ---------------------------------------------------------------- the random family
CAUSES = ("reader_bit", "two_grids", "sum")


class RandomRequantNet(nn.Module):
    """A random integer-simulation net drawn from `seed`: plane 8 or 16, batch 4, widths 8 to 64, bits 2 .. 6, a stem and two to
    four stages.  A stage reads an int8 activation at its grid and draws one kind of Concat:
      "reader_bit"  two convolutions on ONE grid g, the stage's convolution reads at g + d, d != 0
      "two_grids"   two convolutions on grids g and g + d, d != 0, the reader at a bit of its own
      "sum"         Eltwise of two convolutions (now and then with a ReLU) joined with a third convolution, each on a bit of its own
      "served"      two convolutions on one grid, the reader at that grid: the plain rule's Concat
      "declined"    a second convolution reads the Concat at another bit (its output is returned too)
    -- operand bits perturbed so that grids differ --, now and then a ReLU behind the Concat and a MaxPool2d(2) behind the stage.
    `cats`: [(module name, kind)] in execution order."""

    KINDS = ("reader_bit", "two_grids", "sum", "sum", "served", "declined", "reader_bit", "two_grids")

    def __init__(self, seed):
        from concat_nets import conv
        from common.quantity import NewAdd
        super(RandomRequantNet, self).__init__()
        rng = random.Random(3100 + seed)
        self.plane = rng.choice((8, 16))
        widths = (8, 12, 16, 24, 32, 64)
        cin, ib = rng.choice(widths), rng.randint(3, 5)
        self.stem, self.r0 = conv(3, cin, 3, 5, ib, padding=1, seed=seed), nn.ReLU()
        mods, self.stages, self.cats = {}, [], []
        plane = self.plane

        def bit(near, lo=2, hi=6, avoid=None):
            while True:
                b = min(hi, max(lo, near + rng.randint(-2, 2)))
                if avoid is None or b != avoid:
                    return b

        for j in range(rng.choice((2, 3, 3, 4))):
            kind = rng.choice(self.KINDS)
            g = rng.randint(2, 6)
            ca, cb = rng.choice(widths), rng.choice(widths)
            st = {"kind": kind, "relu": rng.random() < 0.4, "pool": plane >= 4 and rng.random() < 0.3, "sum_relu": rng.random() < 0.5}
            if kind == "sum":
                mods["a%d" % j] = conv(cin, ca, 1, ib, g, seed=seed + 10 * j)
                mods["b%d" % j] = conv(cin, ca, 3, ib, bit(g), padding=1, seed=seed + 10 * j + 1)
                mods["add%d" % j], mods["rs%d" % j] = NewAdd(), nn.ReLU()
                mods["c%d" % j] = conv(cin, cb, 1, ib, bit(g), seed=seed + 10 * j + 2)
                rb = bit(g)
            else:
                gb = g if kind in ("reader_bit", "served", "declined") else bit(g, avoid=g)
                mods["a%d" % j] = conv(cin, ca, 1, ib, g, seed=seed + 10 * j)
                mods["b%d" % j] = conv(cin, cb, 3, ib, gb, padding=1, seed=seed + 10 * j + 1)
                rb = g if kind in ("served", "declined") else (bit(g, avoid=g) if kind == "reader_bit" else bit(g))
                if kind == "declined":
                    mods["side%d" % j] = conv(ca + cb, 8, 1, bit(g, avoid=g), 4, seed=seed + 10 * j + 3)
            mods["cat%d" % j], mods["rc%d" % j] = Concat(), nn.ReLU()
            cout, ob = rng.choice(widths), rng.randint(2, 6)
            mods["mix%d" % j], mods["rm%d" % j] = conv(ca + cb, cout, 3, rb, ob, padding=1, seed=seed + 10 * j + 4), nn.ReLU()
            if st["pool"]:
                mods["pool%d" % j] = nn.MaxPool2d(2)
                plane //= 2
            self.stages.append(st)
            self.cats.append(("mods.cat%d" % j, kind))
            cin, ib = cout, ob
        self.mods = nn.ModuleDict(mods)
        self.head = conv(cin, 4, 1, ib, 4, seed=seed + 90)

    def example(self, seed=1):
        return torch.randn(4, 3, self.plane, self.plane, generator=torch.Generator().manual_seed(seed))

    def forward(self, x):
        m, outs = self.mods, []
        x = self.r0(self.stem(x))
        for j, st in enumerate(self.stages):
            a, b = m["a%d" % j](x), m["b%d" % j](x)
            if st["kind"] == "sum":
                s = m["add%d" % j](a, b)
                if st["sum_relu"]:
                    s = m["rs%d" % j](s)
                c = m["cat%d" % j](s, m["c%d" % j](x))
            else:
                c = m["cat%d" % j](a, b)
            if st["kind"] == "declined":
                outs.append(m["side%d" % j](c))
            elif st["relu"]:
                c = m["rc%d" % j](c)
            x = m["rm%d" % j](m["mix%d" % j](c))
            if st["pool"]:
                x = m["pool%d" % j](x)
        return (self.head(x),) + tuple(outs)


SEEDS = list(range(40))


def _model_file(name, path_parts):
    import importlib.util
    import os
    import sys
    mod = sys.modules.get(name)
    if mod is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-quantity_amd", "quantity", "model",
                            *path_parts)
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return mod


def resunet_model(**kw):
    """model/unet/ResUNet_fabu.py's ResUNet (the product's `common` package must be the imported one)."""
    return _model_file("_fq_resunet_fabu", ("unet", "ResUNet_fabu.py")).ResUNet(**kw)
