"""Shared by the windowed average-pool tests (test infrastructure, no product code): the kernel's case list, the rule of
include/fq.h (fq_avgpool_i8_nhwc) in NumPy float32, and small integer-simulation nets built directly from NewConv2d info dicts --
no calibration, so the CPU suite (on the doubles of tests/avgpool_doubles.py) and the GPU suite build the same nets.  Module-level
classes, so a planned net pickles.

Bits: an image at bit 5, activations at bit 4 unless a test says otherwise; a convolution behind a pool reads at the bit of the
pool's source, which is what the calibrator gives it.
"""
import numpy as np
import torch
from torch import nn

from concat_nets import conv, example, DEFAULT_KEYS  # noqa: F401  (shared helpers; re-exported for the tests)

# (N, H, W, C, kh, kw, sh, sw, ph, pw): the smallest shapes at which the kernel can go wrong
KERNEL_CASES = [
    (1, 1, 1, 1, 3, 3, 1, 1, 1, 1),                        # 1x1 plane: one tap, D is 9 or 1
    (1, 2, 2, 16, 3, 3, 1, 1, 1, 1),                       # every window is cut on two sides
    (3, 5, 7, 19, 3, 3, 1, 1, 1, 1),                       # the Inception pool branch; 19 channels: two chunks, one masked
    (1, 9, 11, 100, 3, 3, 2, 2, 1, 1),                     # stride 2 with padding; 7 chunks per pixel
    (1, 9, 11, 19, 3, 3, 2, 2, 0, 0),                      # ... without
    (1, 3, 3, 16, 5, 5, 1, 1, 2, 2),                       # the window is larger than the image
    (3, 5, 7, 19, 2, 2, 2, 2, 0, 0),                       # the transition pool on an odd plane: last row and column dropped
    (1, 2, 2, 1, 2, 2, 2, 2, 0, 0),                        # one output, one channel
    (1, 9, 11, 1, 5, 5, 3, 3, 2, 2),                       # stride 3
    (3, 5, 7, 100, 2, 3, 1, 2, 1, 1),                      # rectangular kernel, stride and padding
    (1, 9, 11, 19, 7, 7, 1, 1, 3, 3),                      # 49 taps
    (1, 16, 8, 19, 8, 8, 8, 8, 0, 0),                      # the 64-tap cap: S reaches +-8192
    (3, 9, 11, 16, 8, 8, 8, 8, 0, 0),                      # ... on a plane it does not divide
]
SHIFTS = (-8, -1, 0, 1, 8)
# more chunks than 2048 x 256 lanes, so that the stride loop runs: 2 x 130 x 130 x 16 chunks = 540 800 > 524 288
STRIDE_LOOP_CASE = (2, 130, 130, 256, 3, 3, 1, 1, 1, 1)


def case_arg(case):
    return ",".join(str(v) for v in case)


def pad16(c):
    return (int(c) + 15) // 16 * 16


def out_plane(case):
    _N, H, W, _C, kh, kw, sh, sw, ph, pw = case
    return (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1


def numpy_rule(x, C, kernel, stride, padding, count_include_pad, shift, relu):
    """include/fq.h's rule on int8 [N, H, W, Cpad] -> int8 [N, P, Q, Cpad]: integer window sums, ONE float32 division by the
    divisor, the exact power of two, rint (half to even), ReLU, clamp; zeros in the padding channels."""
    x = np.asarray(x)
    N, H, W, cpad = x.shape
    (kh, kw), (sh, sw), (ph, pw) = kernel, stride, padding
    P, Q = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    xp = np.pad(x[..., :C].astype(np.int32), ((0, 0), (ph, ph), (pw, pw), (0, 0)))
    inside = np.pad(np.ones((H, W), np.int32), ((ph, ph), (pw, pw)))
    S = np.zeros((N, P, Q, C), np.int32)
    taps = np.zeros((P, Q), np.int32)
    for a in range(kh):
        for b in range(kw):
            S += xp[:, a:a + (P - 1) * sh + 1:sh, b:b + (Q - 1) * sw + 1:sw]
            taps += inside[a:a + (P - 1) * sh + 1:sh, b:b + (Q - 1) * sw + 1:sw]
    D = np.full((P, Q), kh * kw, np.int32) if count_include_pad else taps
    f = S.astype(np.float32) / D.astype(np.float32)[None, :, :, None]
    assert f.dtype == np.float32
    t = f * np.float32(2.0 ** shift)
    r = np.rint(t)
    if relu:
        r = np.maximum(r, np.float32(0))
    out = np.zeros((N, P, Q, cpad), np.int8)
    out[..., :C] = np.clip(r, -128, 127).astype(np.int8)
    return out


def source(rng, case, kind="random"):
    """int8 NHWC source over the whole range (-128 and 127 included) whose padding channels hold non-zero garbage; kind "max" /
    "min": planes of all 127 / all -128 (saturation at positive shifts, S = +-8192 at the cap)."""
    N, H, W, C = case[:4]
    if kind == "random":
        a = rng.integers(-128, 128, size=(N, H, W, pad16(C))).astype(np.int8)
        a.flat[::7] = -128
        a.flat[3::11] = 127
    else:
        a = np.full((N, H, W, pad16(C)), 127 if kind == "max" else -128, np.int8)
    a[..., C:] = np.where(a[..., C:] == 0, 77, a[..., C:]) if kind == "random" else 77
    return a


def tie_source():
    """2x2 / stride 2 windows whose sums are 2, 6, 10, -2, -6, -10, 4, 12, -4 in every channel: S / 4 is k + 0.5 for even and odd k
    at shift 0 (and for the sums 4, 12, -4 at shift -1, for 2, 6, ... at shift 1 twice a half), so half-to-even and
    half-away-from-zero differ.  [1, 6, 6, 16]."""
    sums = np.array([[2, 6, 10], [-2, -6, -10], [4, 12, -4]])
    a = np.zeros((1, 6, 6, 16), np.int8)
    for i in range(3):
        for j in range(3):
            s = int(sums[i, j])
            a[0, 2 * i, 2 * j] = s // 2
            a[0, 2 * i + 1, 2 * j + 1] = s - s // 2
    return a


class InceptionBlockNet(nn.Module):
    """stem + ReLU -> one Inception block (1x1; 1x1 -> 3x3; 1x1 -> 3x3 -> 3x3; AvgPool2d(3, 1, 1) -> 1x1; every layer with its own
    ReLU) joined by three nested Concats -> head.  Every branch reads the stem: with the pool in fp32 form the stem writes fp32."""

    def __init__(self):
        from common.quantity import Concat
        super(InceptionBlockNet, self).__init__()
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.b1, self.rb1 = conv(16, 8, 1, 4, 4), nn.ReLU()
        self.b3r, self.rb3r = conv(16, 8, 1, 4, 4, seed=1), nn.ReLU()
        self.b3, self.rb3 = conv(8, 12, 3, 4, 4, padding=1), nn.ReLU()
        self.bdr, self.rbdr = conv(16, 8, 1, 4, 4, seed=2), nn.ReLU()
        self.bda, self.rbda = conv(8, 8, 3, 4, 4, padding=1), nn.ReLU()
        self.bdb, self.rbdb = conv(8, 8, 3, 4, 4, padding=1, seed=1), nn.ReLU()
        self.pool = nn.AvgPool2d(3, 1, 1)
        self.bp, self.rbp = conv(16, 4, 1, 4, 4), nn.ReLU()
        self.cat1, self.cat2, self.cat3 = Concat(), Concat(), Concat()
        self.head = conv(32, 8, 1, 4, 4)
        self.sources = ("stem",)

    def forward(self, x):
        s = self.r0(self.stem(x))
        a = self.rb1(self.b1(s))
        b = self.rb3(self.b3(self.rb3r(self.b3r(s))))
        d = self.rbdb(self.bdb(self.rbda(self.bda(self.rbdr(self.bdr(s))))))
        p = self.rbp(self.bp(self.pool(s)))
        return self.head(self.cat3(self.cat2(self.cat1(a, b), d), p))


class PoolNet(nn.Module):
    """stem (+ ReLU) -> pool -> reader convolution(s), with what a test varies:
    pool        the nn.AvgPool2d (default: the 2x2 / 2 transition pool)
    relu_behind the ReLU sits BEHIND the pool instead of in front of it (the pool fuses it)
    read_bits   input bits of the readers (one or two convolutions read the pool)
    src_bit     output bit of the stem
    mode        "conv": nothing else; "add_source": the pool reads a NewAdd sum; "concat" / "maxpool" / "foreign": the pool's value
                goes to a Concat / an nn.MaxPool2d / a bare multiplication in front of the reader; "twice": the pool module is called
                a second time on another tensor."""

    def __init__(self, pool=None, relu_behind=False, read_bits=(4,), src_bit=4, mode="conv"):
        from common.quantity import Concat, NewAdd
        super(PoolNet, self).__init__()
        self.stem, self.r0 = conv(3, 16, 3, 5, src_bit, padding=1), nn.ReLU()
        self.pool = nn.AvgPool2d(2) if pool is None else pool
        self.r1 = nn.ReLU()
        cin = 32 if mode == "concat" else 16
        self.c0 = conv(cin, 8, 1, read_bits[0], 4)
        self.c1 = conv(16, 8, 3, read_bits[1], 4, padding=1) if len(read_bits) > 1 else None
        if mode == "add_source":
            self.a, self.b, self.add, self.radd = conv(16, 16, 1, 4, 4), conv(16, 16, 3, 4, 4, padding=1), NewAdd(), nn.ReLU()
        if mode == "concat":
            self.cat = Concat()
        if mode == "maxpool":
            self.mp = nn.MaxPool2d(2)
        if mode == "twice":
            self.mid, self.rmid = conv(16, 16, 1, 4, 4, seed=3), nn.ReLU()
            self.c1 = conv(16, 8, 1, read_bits[0], 4, seed=1)
        self.relu_behind, self.mode = relu_behind, mode
        self.sources = ("stem",)

    def forward(self, x):
        s = self.stem(x)
        if not self.relu_behind:
            s = self.r0(s)
        if self.mode == "add_source":
            s = self.radd(self.add(self.a(s), self.b(s)))
        p = self.pool(s)
        if self.relu_behind:
            p = self.r1(p)
        if self.mode == "concat":
            return self.c0(self.cat(p, s))
        if self.mode == "maxpool":
            return self.c0(self.mp(p))
        if self.mode == "foreign":
            return self.c0(p * 1.0)
        if self.mode == "twice":
            return self.c0(p), self.c1(self.pool(self.rmid(self.mid(s))))
        if self.c1 is not None:
            return self.c0(p), self.c1(p)
        return self.c0(p)


class GlobalPoolNet(nn.Module):
    """A windowed pool AND the whole-plane pool in front of the head: the latter keeps its own forward (_AvgPoolResident)."""

    def __init__(self, size=12):
        from common.quantity import View
        super(GlobalPoolNet, self).__init__()
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.pool = nn.AvgPool2d(2)
        self.c0, self.r1 = conv(16, 8, 1, 4, 4), nn.ReLU()
        self.gpool, self.view = nn.AvgPool2d(size // 2), View()
        self.sources = ("stem",)

    def forward(self, x):
        return self.view(self.gpool(self.r1(self.c0(self.pool(self.r0(self.stem(x)))))))


class G15Net(nn.Module):
    """The FLOAT net calibrated for golden G15 (tests/golden/make_golden_avgpool.py): one Inception-style block with the average
    pool branch and nested Concats, a 2x2 transition pool, a global pool and a classifier.  Input 3 x 12 x 12.  The marker layers
    come from whichever `common.quantity` is imported: the reference's when the golden is captured, the product's in the tests."""

    def __init__(self):
        from common.quantity import Concat, View
        super(G15Net, self).__init__()
        self.stem, self.relu0 = nn.Conv2d(3, 16, 3, padding=1), nn.ReLU(False)
        self.b1, self.relu_b1 = nn.Conv2d(16, 8, 1), nn.ReLU(False)
        self.b3r, self.relu_b3r = nn.Conv2d(16, 8, 1), nn.ReLU(False)
        self.b3, self.relu_b3 = nn.Conv2d(8, 12, 3, padding=1), nn.ReLU(False)
        self.pool_b = nn.AvgPool2d(3, 1, 1)
        self.bp, self.relu_bp = nn.Conv2d(16, 12, 1), nn.ReLU(False)
        self.Concat1, self.Concat2 = Concat(), Concat()
        self.pool_t = nn.AvgPool2d(2)
        self.trans, self.relu_t = nn.Conv2d(32, 16, 1), nn.ReLU(False)
        self.last, self.relu_l = nn.Conv2d(16, 16, 3, padding=1), nn.ReLU(False)
        self.pool_g = nn.AvgPool2d(6)
        self.view = View()
        self.fc = nn.Linear(16, 5)

    def forward(self, x):
        s = self.relu0(self.stem(x))
        a = self.relu_b1(self.b1(s))
        b = self.relu_b3(self.b3(self.relu_b3r(self.b3r(s))))
        p = self.relu_bp(self.bp(self.pool_b(s)))
        c = self.Concat2(self.Concat1(a, b), p)
        t = self.relu_t(self.trans(self.pool_t(c)))
        y = self.relu_l(self.last(t))
        return self.fc(self.view(self.pool_g(y)))


def g15_net():
    return G15Net()


G15_SHAPE = (4, 3, 12, 12)
G15_SEED, G15_CALIB_SEED, G15_INPUT_SEED = 15, 1500, 1515


def inception(size, classes=10, seed=0):
    """model/inception/Inception_fabu.py with seeded weights whose spread keeps the activations alive through its layers."""
    from model.inception.Inception_fabu import InceptionNet
    model = InceptionNet(num_classes=classes, input_size=size)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            fan = max(1, p[0].numel()) if p.dim() > 1 else 1
            p.copy_(torch.randn(p.shape, generator=gen) * ((2.0 / fan) ** 0.5 if p.dim() > 1 else 0.05))
    return model.eval()


def inception_info(model, out_bits, image_bit=5):
    """{layer name: info} for the Inception model above WITHOUT a calibration: output bits from `out_bits` (one float forward's
    abs-max, depthwise_nets.measured_out_bits); the four branch ends of a block share the smallest of their bits (what the nested
    Concats' merge group gives), every layer reads at the bit its producer writes at, and a convolution behind an average pool at
    the bit of the pool's source."""
    from collections import OrderedDict

    from per_channel_chain import numpy_channel_bits
    info = OrderedDict()

    def put(name, ib, ob):
        m = model.get_submodule(name)
        _wb, tensor_bit = numpy_channel_bits(m.weight.detach().cpu().numpy())
        info[name] = {"weight_bit": min(tensor_bit, 12 - ib + ob), "bias_bit": ob, "input_bit": ib, "output_bit": ob, "layer": m,
                      "layer_type": "Conv2d"}
        return ob

    grid = put("conv1.0", image_bit, out_bits["conv1.0"])
    grid = put("conv2.0", grid, out_bits["conv2.0"])
    for n, m in model.features.named_children():
        pre = "features.%s." % n
        if type(m).__name__ != "Inception":
            grid = put(pre + "conv", grid, out_bits[pre + "conv"])
            continue
        ends = (pre + "b1.conv", pre + "b3.conv", pre + "bd.conv_b", pre + "bp.conv")
        out = min(out_bits[e] for e in ends)
        put(ends[0], grid, out)
        put(ends[1], put(pre + "b3.reduce", grid, out_bits[pre + "b3.reduce"]), out)
        a = put(pre + "bd.conv_a", put(pre + "bd.reduce", grid, out_bits[pre + "bd.reduce"]), out_bits[pre + "bd.conv_a"])
        put(ends[2], a, out)
        put(ends[3], grid, out)
        grid = out
    put("classifier.0", grid, out_bits["classifier.0"])
    return info
