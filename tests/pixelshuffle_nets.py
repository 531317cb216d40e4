"""The nets and case lists of the pixel shuffle / unshuffle tests (test infrastructure, no product code).

  pixel_rule(x, C, r, inverse)   the index rule of include/fq.h in numpy on int8 NHWC arrays (padding channels zero).
  kernel_cases() / BIG_CASES / case_arg / model_launches   the cases of tests/test_gpu_pixel_shuffle_i8.py;
                       scripts/pixel_shuffle_geom_check.cpp walks the same shapes.
  ToyNet(variant)      one small integer-simulation net per situation in which enable(pixelshuffle=True) plans a module; built from
                       NewConv2d info dicts, no calibration.
  DeclinedNet(variant) one small net per reason for which a hooked module stays torch's.  DECLINED maps the variant to a piece of
                       its describe().pixelshuffle_left text.
  g27_net()            golden G27: the FLOAT net calibrated by tests/golden/make_golden_pixelshuffle.py.  Imports under the
                       REFERENCE's `common` package too: Eltwise / View come from whichever `common.quantity` is imported.
  RandomPixelShuffleNet(seed)   the random family.
  edsr_model(**kw)     model/edsr/EDSR_fabu.py's EDSR.
"""
import random

import numpy as np
import torch
from torch import nn

import common.quantity as _cq

Concat, Eltwise, View = _cq.Concat, _cq.Eltwise, _cq.View

ALIGNED, GENERAL = 1, 2              # kPsAligned, kPsGeneral of csrc/fq_pixel_shuffle_i8_geom.h
BLOCK, MAX_BLOCKS = 256, 2048        # kPsBlock, kPsMaxBlocks


def pad16(c):
    return (int(c) + 15) // 16 * 16


def family(C, r):
    """The family the geometry header selects, written down independently: the register transpose for r in {2, 4} with
    C % 16 == 0, the byte gather for everything else."""
    return ALIGNED if r in (2, 4) and C % 16 == 0 else GENERAL


def pixel_rule(x, C, r, inverse):
    """x int8 numpy NHWC.  inverse == 0: [N, H, W, pad16(C r^2)] -> [N, H r, W r, pad16(C)] with
    y[n, h r + i, w r + j, c] = x[n, h, w, c r^2 + i r + j]; inverse == 1: [N, H r, W r, pad16(C)] -> [N, H, W, pad16(C r^2)], the inverse
    map.  Padding channels of the result are zero whatever x's hold."""
    N = x.shape[0]
    if not inverse:
        H, W = x.shape[1], x.shape[2]
        assert x.shape[3] == pad16(C * r * r)
        y = np.zeros((N, H * r, W * r, pad16(C)), dtype=np.int8)
        for i in range(r):
            for j in range(r):
                y[:, i::r, j::r, :C] = x[..., i * r + j:C * r * r:r * r]
        return y
    H, W = x.shape[1] // r, x.shape[2] // r
    assert x.shape[3] == pad16(C) and x.shape[1] == H * r and x.shape[2] == W * r
    y = np.zeros((N, H, W, pad16(C * r * r)), dtype=np.int8)
    for i in range(r):
        for j in range(r):
            y[..., i * r + j:C * r * r:r * r] = x[:, i::r, j::r, :C]
    return y


def torch_rule(x, C, r, inverse):
    """The same through torch's own CPU functions on the real channels (NCHW), the padding zero."""
    import torch.nn.functional as F
    real = C if inverse else C * r * r
    t = torch.from_numpy(np.ascontiguousarray(x[..., :real])).permute(0, 3, 1, 2).contiguous()
    t = F.pixel_unshuffle(t, r) if inverse else F.pixel_shuffle(t, r)
    out_c = C * r * r if inverse else C
    y = np.zeros(tuple(t.shape[0:1]) + tuple(t.shape[2:]) + (pad16(out_c),), dtype=np.int8)
    y[..., :out_c] = t.permute(0, 2, 3, 1).numpy()
    return y


# ---------------------------------------------------------------- the kernel's cases: (N, H, W, C, r, inverse), H x W the LOW plane
KERNEL_N = (1, 3)
KERNEL_PLANES = ((1, 1), (2, 3), (5, 4), (8, 8))
KERNEL_CHANNELS = (1, 3, 4, 15, 16, 17, 32, 48, 64, 100)
FACTORS = (2, 3, 4)
# lanes take a second item: 589 824 items of the aligned family, 600 000 of the general one, against 2048 x 256 lanes
BIG_CASES = ((1, 96, 96, 1024, 2, 0), (1, 250, 240, 17, 3, 1))


def kernel_cases(r, inverse):
    return [(N, H, W, C, r, inverse) for N in KERNEL_N for (H, W) in KERNEL_PLANES for C in KERNEL_CHANNELS]


def case_arg(case):
    """The case as scripts/pixel_shuffle_geom_check.cpp reads it: N,H,W/C,r,inverse."""
    return "%d,%d,%d/%d,%d,%d" % tuple(case)


def source(rng, case):
    """The source of a case: int8 over the whole range, the padding channels too -- garbage the kernel must not let through."""
    N, H, W, C, r, inverse = case
    shape = (N, H * r, W * r, pad16(C)) if inverse else (N, H, W, pad16(C * r * r))
    return rng.integers(-128, 128, shape).astype(np.int8)


def model_launches():
    """The launch shapes of scripts/pixelshuffle_cost.py's two models as walker cases, one image each (the batch only repeats the
    plane): EDSR x2 at 96 x 96 and the two stages of EDSR x4; and EDSR x3's, which the GPU tests run at 16 x 16."""
    return [(1, 96, 96, 64, 2, 0), (1, 192, 192, 64, 2, 0), (1, 16, 16, 16, 3, 0), (2, 16, 16, 16, 2, 0)]


def example(n=4, size=8, seed=1):
    return torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------- what is planned
TOY_VARIANTS = ("conv_ps_conv", "relu_ps", "ps_cat", "ps_add", "pu_conv", "yolo", "act_ps", "ps_out")


class ToyNet(nn.Module):
    """stem (3 -> 16, 3x3) + ReLU at bit 4 on the full plane, `down` (16 -> 16, 3x3, stride 2) + ReLU on the half plane, then by
    `variant`:
      "conv_ps_conv"  a (1x1, 16 -> 32) -> PixelShuffle(2) -> head (3x3, 8 -> 8): the aligned family's neighbour, C = 8
      "relu_ps"       a (3x3, 16 -> 36) + ReLU -> PixelShuffle(3) -> head: the ReLU is the convolution's
      "ps_cat"        PixelShuffle(2)(a(down)) joined by a Concat with a skip convolution of the full plane (concat=True)
      "ps_add"        ... added to it by a NewAdd
      "pu_conv"       a (1x1 on the full plane) -> PixelUnshuffle(2) -> head (1x1, 64 -> 8)
      "yolo"          the YOLOv2 passthrough: Concat(PixelUnshuffle(2)(a(full)), b(down)) -> head (concat=True)
      "act_ps"        a -> LeakyReLU -> PixelShuffle(2) -> head at another bit than a's grid (activations=True): the table's lossy
                      value walks through the module to the head
      "ps_out"        a (3x3, 16 -> 12) -> PixelShuffle(2) is the model output (3 channels: an RGB head)
    `fronts`: the producers that go from emit_f32 to integers only; `kw`: further enable() arguments of both arms; `launch`:
    (C, r, inverse) of the module's one launch."""

    def __init__(self, variant):
        from concat_nets import conv
        from common.quantity import NewAdd
        super(ToyNet, self).__init__()
        assert variant in TOY_VARIANTS
        self.variant = v = variant
        self.kw = {}
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.down, self.r1 = conv(16, 16, 3, 4, 4, stride=2, padding=1), nn.ReLU()
        self.fronts = ("a",)
        if v == "conv_ps_conv":
            self.a, self.ps = conv(16, 32, 1, 4, 4), nn.PixelShuffle(2)
            self.head, self.launch = conv(8, 8, 3, 4, 4, padding=1, seed=5), (8, 2, 0)
        elif v == "relu_ps":
            self.a, self.ra, self.ps = conv(16, 36, 3, 4, 3, padding=1), nn.ReLU(), nn.PixelShuffle(3)
            self.head, self.launch = conv(4, 8, 1, 3, 4, seed=5), (4, 3, 0)
        elif v in ("ps_cat", "ps_add"):
            self.a, self.ps = conv(16, 64, 1, 4, 4), nn.PixelShuffle(2)
            self.skip = conv(16, 16, 1, 4, 4, seed=2)
            if v == "ps_cat":
                self.cat, self.kw = Concat(), dict(concat=True)
            else:
                self.add = NewAdd()
            self.head, self.launch = conv(32 if v == "ps_cat" else 16, 8, 1, 4, 4, seed=5), (16, 2, 0)
            self.fronts = ("a", "skip") if v == "ps_add" else ("a",)
        elif v == "pu_conv":
            self.a, self.ps = conv(16, 16, 1, 4, 4), nn.PixelUnshuffle(2)
            self.head, self.launch = conv(64, 8, 1, 4, 4, seed=5), (16, 2, 1)
        elif v == "yolo":
            self.a, self.ps = conv(16, 5, 1, 4, 4), nn.PixelUnshuffle(2)
            self.b = conv(16, 12, 1, 4, 4, seed=2)
            self.cat, self.kw = Concat(), dict(concat=True)
            self.head, self.launch = conv(32, 8, 1, 4, 4, seed=5), (5, 2, 1)
        elif v == "act_ps":
            self.a, self.act, self.ps = conv(16, 32, 1, 4, 4), nn.LeakyReLU(0.1), nn.PixelShuffle(2)
            self.head, self.launch, self.kw = conv(8, 8, 3, 3, 4, padding=1, seed=5), (8, 2, 0), dict(activations=True)
        else:
            self.a, self.ps, self.launch = conv(16, 12, 3, 4, 4, padding=1), nn.PixelShuffle(2), (3, 2, 0)

    def forward(self, x):
        v = self.variant
        s = self.r0(self.stem(x))
        d = self.r1(self.down(s))
        if v == "conv_ps_conv":
            return self.head(self.ps(self.a(d)))
        if v == "relu_ps":
            return self.head(self.ps(self.ra(self.a(d))))
        if v == "ps_cat":
            return self.head(self.cat(self.ps(self.a(d)), self.skip(s)))
        if v == "ps_add":
            return self.head(self.add(self.ps(self.a(d)), self.skip(s)))
        if v == "pu_conv":
            return self.head(self.ps(self.a(s)))
        if v == "yolo":
            return self.head(self.cat(self.ps(self.a(s)), self.b(d)))
        if v == "act_ps":
            return self.head(self.ps(self.act(self.a(d))))
        return self.ps(self.a(d))


# ---------------------------------------------------------------- what is declined
DECLINED = {
    "sum": "NewAdd sum (int16)", "fp32_source": "no integer form", "twice": "more than once", "nd": "not 4-D",
    "factor": "factor 5", "geometry": "unsupported geometry",
}


class DeclinedNet(nn.Module):
    """A 3 -> 16 stem + ReLU at bit 4, a (1x1, 16 -> 100 or 32) on grid 4, `ps` and a 1x1 head -- planned as it stands ("ok") -- and by
    `variant` one thing that leaves `ps` torch's (the keys of DECLINED).  "geometry" is the "ok" net: the test makes
    _native.pixel_shuffle_supported refuse.  "nd" is a chain of two Linear layers on a 3-D input [4, T, F], whose output torch's
    module reads as (C, H, W); it runs on the CPU doubles only (the library's fp32 tail reads channels at dim 1).  Module-level, so the
    planned net pickles."""

    def __init__(self, variant):
        from concat_nets import conv
        from common.quantity import NewAdd, NewLinear
        super(DeclinedNet, self).__init__()
        assert variant == "ok" or variant in DECLINED
        self.variant = v = variant
        if v == "nd":
            gen = torch.Generator().manual_seed(7)
            l1, l2 = nn.Linear(6, 8), nn.Linear(16, 4)
            with torch.no_grad():
                for lin in (l1, l2):
                    lin.weight.copy_(torch.randn(lin.weight.shape, generator=gen) * 0.4)
                    lin.bias.copy_(torch.randn(lin.bias.shape, generator=gen) * 0.2)
            info = {"weight_bit": 6, "bias_bit": 4, "input_bit": 4, "output_bit": 4}
            self.l1, self.ps, self.l2 = NewLinear(l1, dict(info)), nn.PixelShuffle(2), NewLinear(l2, dict(info))
            return
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        r = 5 if v == "factor" else 2
        self.a, self.ps = conv(16, 100 if v == "factor" else 32, 1, 4, 4), nn.PixelShuffle(r)
        width = 4 if v == "factor" else 8
        if v == "sum":
            self.b, self.add = conv(16, 32, 3, 4, 3, padding=1, seed=3), NewAdd()
        if v == "fp32_source":
            self.ceil = nn.MaxPool2d(3, 1, 1, ceil_mode=True)
        self.head = conv(2 if v == "twice" else width, 8, 1, 4, 4, seed=9)

    def example(self, seed=1):
        gen = torch.Generator().manual_seed(seed)
        return torch.randn(4, 5, 6, generator=gen) if self.variant == "nd" else torch.randn(4, 3, 8, 8, generator=gen)

    def forward(self, x):
        v = self.variant
        if v == "nd":
            return self.l2(self.ps(self.l1(x)))
        s = self.r0(self.stem(x))
        a = self.a(s)
        if v == "sum":
            a = self.add(a, self.b(s))
        if v == "fp32_source":
            a = self.ceil(a)                                  # (a ceil_mode max-pool is traced but not planned: its value is fp32)
        y = self.ps(a)
        if v == "twice":
            y = self.ps(y)
        return self.head(y)


# ---------------------------------------------------------------- golden G27
G27_SHAPE = (4, 3, 16, 16)
G27_SEED, G27_CALIB_SEED, G27_INPUT_SEED = 27, 2700, 2727


class G27Net(nn.Module):
    """The FLOAT net calibrated for golden G27: conv1 + ReLU (16 px, 8 ch) -> PixelUnshuffle(2) (8 px, 32 ch) -> conv2 + ReLU ->
    one residual step Eltwise(conv4(ReLU(conv3(.))), .) -> conv5 to 4 * 8 channels -> PixelShuffle(2) (16 px, 8 ch) -> conv6: the image
    [N, 3, 16, 16]."""

    def __init__(self):
        super(G27Net, self).__init__()
        self.conv1, self.relu1 = nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(False)
        self.unshuffle = nn.PixelUnshuffle(2)
        self.conv2, self.relu2 = nn.Conv2d(32, 16, 3, 1, 1), nn.ReLU(False)
        self.conv3, self.relu3 = nn.Conv2d(16, 16, 3, 1, 1), nn.ReLU(False)
        self.conv4 = nn.Conv2d(16, 16, 3, 1, 1)
        self.Eltwise1 = Eltwise()
        self.conv5 = nn.Conv2d(16, 32, 3, 1, 1)
        self.shuffle = nn.PixelShuffle(2)
        self.conv6 = nn.Conv2d(8, 3, 3, 1, 1)

    def forward(self, x):
        x = self.relu2(self.conv2(self.unshuffle(self.relu1(self.conv1(x)))))
        x = self.Eltwise1(self.conv4(self.relu3(self.conv3(x))), x)
        return self.conv6(self.shuffle(self.conv5(x)))


def g27_net():
    return G27Net()


# ---------------------------------------------------------------- the random family
class RandomPixelShuffleNet(nn.Module):
    """A random integer-simulation net drawn from `seed`: low-resolution plane 4 to 16, batch 4, widths 4 to 64, bits 2 .. 6, a stem
    and two to four stages.  A stage reads an int8 activation and draws one module:
      "ps"       convolution to C r^2 channels (now and then with a ReLU) -> PixelShuffle(r) -> the stage's convolution
      "pu"       PixelUnshuffle(r) of the stage's input (where r divides the plane) -> the stage's convolution
      "ps_pu"    PixelShuffle(r) -> PixelUnshuffle(r): one module reads the other
      "ps_relu"  a ReLU directly behind the PixelShuffle: it reads the fp32 form
      "sum"      PixelShuffle of an Eltwise of two convolutions: declined (int16)
    with the reading convolution now and then at another bit than the module's grid, so that it reads fp32.  `mods`: [(module
    name, "ps" | "pu", r, expected to be planned)] in execution order."""

    KINDS = ("ps", "pu", "ps", "pu", "ps_pu", "ps_relu", "sum", "ps", "pu")

    def __init__(self, seed):
        from concat_nets import conv
        from common.quantity import NewAdd
        super(RandomPixelShuffleNet, self).__init__()
        rng = random.Random(3200 + seed)
        self.plane = plane = rng.choice((4, 6, 8, 12, 16))
        widths = (4, 8, 12, 16, 32, 64)
        cin, ib = rng.choice(widths), rng.randint(3, 5)
        self.stem, self.r0 = conv(3, cin, 3, 5, ib, padding=1, seed=seed), nn.ReLU()
        mods, self.stages, self.mods_drawn = {}, [], []
        for j in range(rng.choice((2, 3, 3, 4))):
            kind = rng.choice(self.KINDS)
            r = rng.choice((2, 3, 4))
            if kind != "pu" and plane * r > 48:               # (keep the planes small: the CPU doubles convolve in fp32)
                r = 2
                if plane * r > 48:
                    kind = "pu"
            if kind == "pu" and (plane % r or plane // r < 2):
                r = next((q for q in (2, 3, 4) if plane % q == 0 and plane // q >= 2), None)
                kind = "ps" if r is None else kind
                r = r or 2
            g = rng.randint(2, 6)
            st = {"kind": kind, "r": r, "relu": rng.random() < 0.5}
            c = rng.choice((3, 4, 8, 16))                     # the shallow width of a shuffle
            if kind in ("ps", "ps_pu", "ps_relu", "sum"):
                mods["a%d" % j] = conv(cin, c * r * r, 1, ib, g, seed=seed + 10 * j)
                if kind == "sum":
                    mods["b%d" % j], mods["add%d" % j] = conv(cin, c * r * r, 3, ib, g, padding=1, seed=seed + 10 * j + 1), NewAdd()
                mods["ra%d" % j], mods["ps%d" % j] = nn.ReLU(), nn.PixelShuffle(r)
                self.mods_drawn.append(("mods.ps%d" % j, "ps", r, kind != "sum"))
                width = c
                if kind == "ps_pu":
                    mods["pu%d" % j] = nn.PixelUnshuffle(r)
                    self.mods_drawn.append(("mods.pu%d" % j, "pu", r, True))
                    width = c * r * r
                elif kind == "ps_relu":
                    mods["rp%d" % j] = nn.ReLU()
                    plane *= r
                else:
                    plane *= r
            else:
                mods["pu%d" % j] = nn.PixelUnshuffle(r)
                self.mods_drawn.append(("mods.pu%d" % j, "pu", r, True))
                width, g = cin * r * r, ib
                plane //= r
            rb = g if rng.random() < 0.8 else (g + 1 if g < 6 else g - 1)
            cout, ob = rng.choice(widths), rng.randint(2, 6)
            mods["mix%d" % j], mods["rm%d" % j] = conv(width, cout, 3, rb, ob, padding=1, seed=seed + 10 * j + 4), nn.ReLU()
            self.stages.append(st)
            cin, ib = cout, ob
        self.mods = nn.ModuleDict(mods)
        self.head = conv(cin, 4, 1, ib, 4, seed=seed + 90)

    def example(self, seed=1):
        return torch.randn(4, 3, self.plane, self.plane, generator=torch.Generator().manual_seed(seed))

    def forward(self, x):
        m = self.mods
        x = self.r0(self.stem(x))
        for j, st in enumerate(self.stages):
            kind = st["kind"]
            if kind == "pu":
                x = m["pu%d" % j](x)
            else:
                a = m["a%d" % j](x)
                if kind == "sum":
                    a = m["add%d" % j](a, m["b%d" % j](x))
                elif st["relu"]:
                    a = m["ra%d" % j](a)
                x = m["ps%d" % j](a)
                if kind == "ps_pu":
                    x = m["pu%d" % j](x)
                elif kind == "ps_relu":
                    x = m["rp%d" % j](x)
            x = m["rm%d" % j](m["mix%d" % j](x))
        return self.head(x)


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


def edsr_model(**kw):
    """model/edsr/EDSR_fabu.py's EDSR (the product's `common` package must be the imported one)."""
    return _model_file("_fq_edsr_fabu", ("edsr", "EDSR_fabu.py")).EDSR(**kw)
