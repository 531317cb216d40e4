"""The nets and case lists of the table-activation tests (test infrastructure, no product code).

  ACTIVATIONS          {listed type name: a constructor of one module of it}, the names appended to tools/configs.yml.
  g21_net()            golden G21: conv -> LeakyReLU(0.1) -> MaxPool -> conv -> Hardswish -> two overlapping Slices (a pure permutation
                       would keep the reference's value fingerprint) joined by a Concat -> conv (stride 2) -> SiLU -> nearest upsampling x2 -> Concat with the first Concat -> conv ->
                       ReLU, a pool, View and a Linear.  Imports under the REFERENCE's `common` package too (the golden script):
                       Concat / View come from whichever `common.quantity` is imported, Slice from shuffle_nets.
  integer_weights(m)   FIXED weights: the stem is dense on the integer image; every convolution BEHIND an activation has one tap
                       of +-1 per output channel and an integer bias, so that its fp32 result is one product plus one bias --
                       the same bits in every engine whatever the order of its sums, though its input is no integer any more.
  RefusalNet(variant)  one small integer-simulation net per case the lossy-value rule refuses, built from NewConv2d info dicts.
  KERNEL_CASES         (N, H, W, C, Cpad) of tests/test_gpu_activation_i8.py; scripts/act_lut_geom_check.cpp walks the same list.
  act_lut_rule         the kernel's rule in numpy.
"""
import zlib

import numpy as np
import torch
from torch import nn

import common.quantity as _cq
from shuffle_nets import Slice, integer_batches, integer_input  # noqa: F401

Concat, View = _cq.Concat, _cq.View

ACTIVATIONS = {
    "LeakyReLU": lambda: nn.LeakyReLU(0.1), "PReLU": lambda: nn.PReLU(1, 0.25), "Hardswish": nn.Hardswish,
    "Hardsigmoid": nn.Hardsigmoid, "SiLU": nn.SiLU, "Sigmoid": nn.Sigmoid, "Tanh": nn.Tanh, "ELU": lambda: nn.ELU(1.0),
    "Hardtanh": lambda: nn.Hardtanh(-1.0, 2.0), "Mish": nn.Mish, "GELU": nn.GELU,
}
GRID_BIT_PAIRS = ((4, 4), (5, 3), (2, 6), (-1, 0))

G21_SHAPE = (4, 3, 16, 16)
G21_SEED, G21_CALIB_SEED, G21_INPUT_SEED = 21, 2100, 2121
G21_ACTS = ("act1", "act2", "act3")


class G21Net(nn.Module):

    def __init__(self):
        super(G21Net, self).__init__()
        self.conv1, self.act1 = nn.Conv2d(3, 8, 3, 1, 1), nn.LeakyReLU(0.1)
        self.pool = nn.MaxPool2d(2)
        self.conv2, self.act2 = nn.Conv2d(8, 12, 3, 1, 1), nn.Hardswish()
        self.left, self.right, self.Concat1 = Slice(2, 10), Slice(6, 12), Concat()
        self.conv3, self.act3 = nn.Conv2d(14, 10, 3, 2, 1), nn.SiLU()
        self.up, self.Concat2 = nn.UpsamplingNearest2d(scale_factor=2), Concat()
        self.conv4, self.relu4 = nn.Conv2d(24, 16, 1, 1, 0), nn.ReLU(False)
        self.avgpool, self.view, self.fc = nn.AvgPool2d(8), View(), nn.Linear(16, 10)

    def forward(self, x):
        a = self.act2(self.conv2(self.pool(self.act1(self.conv1(x)))))
        c = self.Concat1(self.right(a), self.left(a))
        u = self.up(self.act3(self.conv3(c)))
        return self.fc(self.view(self.avgpool(self.relu4(self.conv4(self.Concat2(u, c))))))


def g21_net():
    return G21Net()


def integer_weights(model, base_seed=G21_SEED, dense=("conv1", "stem")):
    sd = model.state_dict()
    with torch.no_grad():
        for key in sorted(sd.keys()):
            t = sd[key]
            g = np.random.default_rng(base_seed * 1000003 + zlib.crc32(key.encode()))
            shape = tuple(t.shape)
            if t.dim() <= 1:                                  # a bias (an nn.PReLU weight keeps its value)
                if key.endswith("bias"):
                    t.copy_(torch.from_numpy(g.integers(-2, 3, shape).astype(np.float32)))
                continue
            if t.dim() == 4 and key.split(".")[0] not in dense:      # one tap of +-1 per output channel
                v = np.zeros(shape, dtype=np.float32)
                k = shape[2] * shape[3]
                tap = g.integers(0, k, shape[0])
                v[np.arange(shape[0]), g.integers(0, shape[1], shape[0]), tap // shape[3], tap % shape[3]] = \
                    np.where(g.random(shape[0]) < 0.7, 1, -1)
            else:                                             # dense: sparse, entries in [-2, 2]
                keep = min(1.0, 6.0 / int(np.prod(shape[1:])))
                v = (g.integers(-2, 3, shape) * (g.random(shape) < keep)).astype(np.float32)
            t.copy_(torch.from_numpy(v))
    return model


# ---------------------------------------------------------------- the kernel's rule and the shapes it is run on
BLOCK, MAX_BLOCKS = 256, 2048            # kActLutBlock, kActLutMaxBlocks of csrc/fq_act_lut_i8_geom.h


def pad16(c):
    return (int(c) + 15) // 16 * 16


def act_lut_rule(x, c, table):
    """y[..., j] = table[x[..., j] + 128] for j < c, zero behind; x int8 [..., Cpad], table int8 [256] (numpy)."""
    y = np.zeros_like(x)
    y[..., :c] = table[x[..., :c].astype(np.int32) + 128]
    return y


# the project's padding ...
KERNEL_CASES = [(2, 5, 5, c, pad16(c)) for c in (1, 3, 5, 58, 64)] + [(1, 1, 1, 3, 16), (3, 17, 9, 116, 128)]
# ... rows that are no multiple of 16 bytes, so that the bytes behind the last whole chunk go one by one
KERNEL_CASES += [(2, 5, 5, 3, 3), (2, 5, 5, 3, 5), (1, 1, 1, 3, 3), (3, 17, 9, 58, 61), (1, 1, 7, 1, 1)]
# ... and the smallest tensor that takes every workgroup through its loop twice (one chunk more than one pass of the capped grid)
STRIDE_LOOP = (1, 1, BLOCK * MAX_BLOCKS + 1, 5, 16)
KERNEL_CASES.append(STRIDE_LOOP)


def case_arg(case):
    return "%d,%d,%d,%d,%d" % case


# ---------------------------------------------------------------- what the lossy-value rule refuses
REFUSALS = ("add", "avgpool", "cat_grid", "bare_cat", "output", "two_bits", "prelu_channels", "twice", "inplace")


class RefusalNet(nn.Module):
    """A 3 -> 16 stem + ReLU at bit 4, a 1x1 `mid` (output grid 4) and the activation `act` behind it, then by `variant`:
      "add"             act -> NewAdd with the stem's output                    "avgpool"   act -> AvgPool2d(3, 1, 1) -> conv
      "cat_grid"        act -> Concat whose other operand is on grid 3          "bare_cat"  act -> a bare torch.cat
      "output"          act is a model output (next to the head's)              "two_bits"  act -> convolutions at input bits 4 and 3
      "prelu_channels"  an nn.PReLU with one weight per channel                 "twice"     the module called twice
      "inplace"         nn.Hardswish(inplace=True)                              "ok"        act -> conv: planned
    A module-level class, so the rebuilt model pickles."""

    def __init__(self, variant, act=None):
        from concat_nets import conv
        from common.quantity import NewAdd
        super(RefusalNet, self).__init__()
        self.variant = variant
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.mid = conv(16, 16, 1, 4, 4)
        if act is not None:
            self.act = act
        elif variant == "prelu_channels":
            self.act = nn.PReLU(16, 0.25)
        else:
            self.act = nn.Hardswish(inplace=True) if variant == "inplace" else nn.Hardswish()
        if variant == "add":
            self.add = NewAdd()
        if variant == "avgpool":
            self.avg = nn.AvgPool2d(3, 1, 1)
        if variant == "cat_grid":
            self.other, self.cat = conv(16, 8, 1, 4, 3, seed=5), Concat()
        if variant == "two_bits":
            self.side = conv(16, 8, 1, 3, 4, seed=7)
        cin = {"cat_grid": 24, "bare_cat": 32}.get(variant, 16)
        self.head = conv(cin, 8, 1, 4, 4, seed=9)

    def forward(self, x):
        s = self.r0(self.stem(x))
        a = self.act(self.mid(s))
        v = self.variant
        if v == "add":
            return self.head(self.add(a, s))
        if v == "avgpool":
            return self.head(self.avg(a))
        if v == "cat_grid":
            return self.head(self.cat(a, self.other(s)))
        if v == "bare_cat":
            return self.head(torch.cat((a, s), 1))
        if v == "output":
            return self.head(a), a
        if v == "two_bits":
            return self.head(a) + self.side(a)
        if v == "twice":
            return self.head(self.act(a))
        return self.head(a)


def yolo_model(**kw):
    """model/yolotiny/YoloTiny_fabu.py's YoloTiny (the product's `common` package must be the imported one)."""
    import importlib.util
    import os
    import sys
    name = "_fq_yolotiny_fabu"
    mod = sys.modules.get(name)
    if mod is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-quantity_amd", "quantity", "model",
                            "yolotiny", "YoloTiny_fabu.py")
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return mod.YoloTiny(**kw)


class RandomActNet(nn.Module):
    """The generator of scripts/recon_fuzz.py's `act` mode: a 3x3 stem + ReLU, then one to four steps of a random convolution
    (1x1 or 3x3, 8 to 24 channels) with a random listed activation behind it -- now and then inplace=True, which the plan must leave -- and behind some of them a 2x2 max-pool, a Slice, or two overlapping Slices joined by a
    Concat; then a 1x1 + ReLU, a global average pool, View and a Linear.  Seeded weights.  A module-level class, so the rebuilt
    model pickles; `cin`, `size`, `batch` and `n` are what recon_fuzz reads."""

    def __init__(self, i, seed):
        super(RandomActNet, self).__init__()
        rng = np.random.default_rng(100003 * seed + i)
        self.cin, self.batch = 3, 4
        self.size = size = int(rng.choice((8, 16)))
        c = int(rng.choice((8, 16)))
        self.stem, self.r0 = nn.Conv2d(3, c, 3, 1, 1), nn.ReLU(False)
        self.steps = []
        names = [n for n in ACTIVATIONS if n != "PReLU"]     # (a module with a weight does not go through the calibration flow)
        for k in range(int(rng.integers(1, 5))):
            cout = int(rng.choice((8, 12, 16, 20, 24)))
            ks = int(rng.choice((1, 3)))
            setattr(self, "conv%d" % k, nn.Conv2d(c, cout, ks, 1, ks // 2))
            name = names[int(rng.integers(len(names)))]
            act = ACTIVATIONS[name]()
            roll = rng.random()
            if roll < 0.15 and hasattr(act, "inplace"):
                act.inplace = True
            setattr(self, "act%d" % k, act)
            c = cout
            behind = str(rng.choice(("none", "none", "pool", "slice", "cat")))
            if behind == "pool" and size >= 4:
                setattr(self, "pool%d" % k, nn.MaxPool2d(2))
                size //= 2
            elif behind == "slice":
                a = int(rng.integers(0, c // 2))
                setattr(self, "slice%d" % k, Slice(a, a + c // 2))
                c = c // 2
            elif behind == "cat":
                a, b = int(rng.integers(1, c // 2)), int(rng.integers(c // 2, c))
                setattr(self, "left%d" % k, Slice(a, c))
                setattr(self, "right%d" % k, Slice(0, b))
                setattr(self, "Concat%d" % k, Concat())
                c = (c - a) + b
            else:
                behind = "none"
            self.steps.append((k, behind))
        self.last, self.r1 = nn.Conv2d(c, 16, 1), nn.ReLU(False)
        self.avgpool, self.view, self.fc = nn.AvgPool2d(size), View(), nn.Linear(16, 10)
        self.n = len(list(self.modules()))
        gen = torch.Generator().manual_seed(1000 * seed + i)
        with torch.no_grad():
            for p in self.parameters():
                if p.dim() > 1:
                    p.copy_(torch.randn(p.shape, generator=gen) * (1.5 / max(1, p[0].numel()) ** 0.5))
                else:
                    p.copy_(torch.randn(p.shape, generator=gen) * 0.2)

    def forward(self, x):
        x = self.r0(self.stem(x))
        for k, behind in self.steps:
            x = getattr(self, "act%d" % k)(getattr(self, "conv%d" % k)(x))
            if behind == "pool":
                x = getattr(self, "pool%d" % k)(x)
            elif behind == "slice":
                x = getattr(self, "slice%d" % k)(x)
            elif behind == "cat":
                x = getattr(self, "Concat%d" % k)(getattr(self, "left%d" % k)(x), getattr(self, "right%d" % k)(x))
        return self.fc(self.view(self.avgpool(self.r1(self.last(x)))))
