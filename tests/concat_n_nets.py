"""Shared by the N-source Concat tests (test infrastructure, no product code): the kernel's case list, the index rule of
include/fq.h (fq_concat_n_i8_nhwc) in NumPy, and small integer-simulation nets with nested Concat markers built directly from
NewConv2d info dicts (concat_nets.conv) -- no calibration, so the CPU suite (on the doubles of tests/concat_n_doubles.py) and the
GPU suite build the same nets and run the same checks (check_net).  Module-level classes, so a planned net pickles.

Bits: an image at bit 5, every activation at bit 4: all operands of all Concats of a net sit on one grid.
"""
import numpy as np
import torch
from torch import nn

import avgpool_nets as an
import concat_nets as cn
from concat_nets import conv, example  # noqa: F401

# (N, H, W, [C...], [up...]); H, W are the OUTPUT plane.  ReLU flags: relu_patterns() below.
ALIGNED_CASES = [(2, 5, 7, [16, 32, 16, 48], [1, 1, 1, 1]), (1, 4, 4, [16] * 8, [1] * 8)]
GENERAL_CASES = [
    (3, 7, 9, [20, 44, 13], [1, 1, 1]),
    (1, 6, 6, [17, 1, 30], [1, 1, 1]),                                      # a one-channel source in the middle
    (2, 3, 5, [3, 5, 1, 2, 4, 1, 7, 6], [1] * 8),                           # eight sources, six of them inside chunk 0
    (1, 2, 2, [13, 2, 1], [1, 1, 1]),                                       # sum C == 16: no output padding
    (1, 1, 1, [1, 1, 1], [1, 1, 1]),
]
UPSAMPLED_CASES = [
    (2, 8, 12, [24, 8, 16], [1, 2, 4]), (1, 8, 8, [5, 7, 9], [2, 1, 4]), (2, 4, 6, [20, 44, 13], [1, 2, 1]),
    (1, 8, 8, [16, 16, 32], [4, 2, 1]),
]
# more than 2048 * 256 chunks, so that the lanes stride over the pixels: aligned with CH = 16, general with CH = 5 (a stride the
# chunk count does not divide).  The only cases above a few hundred kilobytes.
STRIDED_CASES = [(9, 64, 64, [64, 64, 64, 64], [1, 1, 1, 1]), (8, 128, 112, [20, 44, 13], [1, 1, 1])]
# every case of the two-source kernel's list goes through the new entry point as well
OLD_CASES = [(N, H, W, [C0] + ([C1] if C1 else []), [u0] + ([u1] if C1 else [])) for (N, H, W, C0, C1, u0, u1) in cn.KERNEL_CASES]
NEW_CASES = ALIGNED_CASES + GENERAL_CASES + UPSAMPLED_CASES
KERNEL_CASES = NEW_CASES + STRIDED_CASES + OLD_CASES


def relu_patterns(case):
    """ReLU flags a case runs with: the general cases all 0, all 1 and mixed (1, 0, 1, ...); every other case all 0 and mixed."""
    n = len(case[3])
    mixed = [(i + 1) % 2 for i in range(n)]
    if case in GENERAL_CASES:
        return [[0] * n, [1] * n, mixed]
    if case in STRIDED_CASES:
        return [mixed]
    return [[0] * n, mixed] if n > 1 or case[4][0] > 1 else [[1]]


def case_arg(case):
    return "%d,%d,%d/%s/%s" % (case[0], case[1], case[2], ",".join(str(c) for c in case[3]), ",".join(str(u) for u in case[4]))


def case_id(case):
    return "n%d_%dx%d_c%s_up%s" % (case[0], case[1], case[2], "-".join(str(c) for c in case[3]), "".join(str(u) for u in case[4]))


def pad16(c):
    return (int(c) + 15) // 16 * 16


def sources(rng, case):
    """int8 NHWC sources over the whole range (-128 and 127 included) whose padding channels hold non-zero garbage."""
    N, H, W, Cs, ups = case
    out = []
    for C, u in zip(Cs, ups):
        a = rng.integers(-128, 128, size=(N, H // u, W // u, pad16(C))).astype(np.int8)
        a.flat[::7] = -128
        a.flat[3::11] = 127
        a[..., C:] = np.where(a[..., C:] == 0, 77, a[..., C:])
        out.append(a)
    return out


def index_rule(case, arrays, relus):
    """include/fq.h's rule, element by element of the index arithmetic."""
    N, H, W, Cs, ups = case
    want = np.zeros((N, H, W, pad16(sum(Cs))), dtype=np.int8)
    hh, ww = np.arange(H), np.arange(W)
    base = 0
    for a, C, u, r in zip(arrays, Cs, ups, relus):
        part = a[:, hh // u][:, :, ww // u][..., :C]
        want[..., base:base + C] = np.maximum(part, 0) if r else part
        base += C
    return want


# ---------------------------------------------------------------- nets
class SppNet(nn.Module):
    """conv + ReLU -> its value, MaxPool2d(5, 1, 2) and MaxPool2d(9, 1, 4) of it joined by two nested Concats -> conv."""

    def __init__(self):
        from common.quantity import Concat
        super(SppNet, self).__init__()
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.p5, self.p9 = nn.MaxPool2d(5, 1, 2), nn.MaxPool2d(9, 1, 4)
        self.cat1, self.cat2 = Concat(), Concat()
        self.head = conv(48, 8, 1, 4, 4)

    def forward(self, x):
        s = self.r0(self.stem(x))
        return self.head(self.cat2(self.cat1(s, self.p5(s)), self.p9(s)))


class ChainNet(nn.Module):
    """A DenseNet-style accumulation: `leaves` 1x1 branches of 4 channels joined by a chain of leaves - 1 Concats -> conv."""

    def __init__(self, leaves=9):
        from common.quantity import Concat
        super(ChainNet, self).__init__()
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.branches = nn.ModuleList([conv(16, 4, 1, 4, 4, seed=i) for i in range(leaves)])
        self.cats = nn.ModuleList([Concat() for _ in range(leaves - 1)])
        self.head = conv(4 * leaves, 8, 1, 4, 4)

    def forward(self, x):
        s = self.r0(self.stem(x))
        acc = self.branches[0](s)
        for b, cat in zip(self.branches[1:], self.cats):
            acc = cat(acc, b(s))
        return self.head(acc)


class NestedNet(nn.Module):
    """cat2(inner, c) with inner = [ReLU](cat1(a, b)); no branch has a ReLU of its own, so negative integers reach the Concats.
    inner_relu  the inner Concat has its own nn.ReLU and the outer one none: the mixed-flag case
    side        a second convolution reads the inner Concat as well: it is not deferred
    up          a nearest upsampling by 2 sits between the two Concats (the branches a, b run on the half plane)"""

    def __init__(self, inner_relu=False, side=False, up=False):
        from common.quantity import Concat
        super(NestedNet, self).__init__()
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.down = conv(16, 16, 3, 4, 4, stride=2, padding=1, seed=3) if up else None
        self.a, self.b, self.c = conv(16, 8, 1, 4, 4), conv(16, 8, 3, 4, 4, padding=1), conv(16, 8, 1, 4, 4, seed=1)
        self.cat1, self.cat2 = Concat(), Concat()
        self.r1 = nn.ReLU() if inner_relu else None
        self.up = nn.UpsamplingNearest2d(scale_factor=2) if up else None
        self.side = conv(16, 8, 1, 4, 4, seed=2) if side else None
        self.head = conv(24, 8, 1, 4, 4)

    def forward(self, x):
        s = self.r0(self.stem(x))
        t = self.down(s) if self.down is not None else s
        inner = self.cat1(self.a(t), self.b(t))
        if self.r1 is not None:
            inner = self.r1(inner)
        y = self.head(self.cat2(self.up(inner) if self.up is not None else inner, self.c(s)))
        return (y, self.side(inner)) if self.side is not None else y


TWO, NSRC = "concat_i8_nhwc", "concat_n_i8_nhwc"
# tag -> (net, flattened_concats, resident_concats, [launches of one forward with flatten=True: (entry point, [(C, up, relu)...])],
#         names of the deferred Concats).  The two-source entry point has ONE ReLU flag: it is written to every operand here.
NETS = {
    "inception_block": (an.InceptionBlockNet, 2, 3, [(NSRC, [(8, 1, 0), (12, 1, 0), (8, 1, 0), (4, 1, 0)])], ("cat1", "cat2")),
    "spp": (SppNet, 1, 2, [(NSRC, [(16, 1, 0), (16, 1, 0), (16, 1, 0)])], ("cat1",)),
    "chain_of_nine": (ChainNet, 6, 8, [(NSRC, [(4, 1, 0)] * 8), (TWO, [(32, 1, 0), (4, 1, 0)])], tuple("cats.%d" % i for i in range(6))),
    "inner_relu": (lambda: NestedNet(inner_relu=True), 1, 2, [(NSRC, [(8, 1, 1), (8, 1, 1), (8, 1, 0)])], ("cat1",)),
    "second_reader": (lambda: NestedNet(side=True), 0, 2, [(TWO, [(8, 1, 0), (8, 1, 0)]), (TWO, [(16, 1, 0), (8, 1, 0)])], ()),
    "upsampling_between": (lambda: NestedNet(up=True), 0, 2, [(TWO, [(8, 1, 0), (8, 1, 0)]), (TWO, [(16, 2, 0), (8, 1, 0)])], ()),
}


def _tuple(t):
    return t if isinstance(t, tuple) else (t,)


def same(a, b):
    a, b = _tuple(a), _tuple(b)
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


class Recorder(object):
    """Wraps the two Concat entry points of `nat` and records (entry point, [(C, up, relu)...]) of every launch."""

    def __init__(self, nat):
        self.nat, self.calls, self.real = nat, [], {}

    def __enter__(self):
        self.real = {TWO: getattr(self.nat, TWO), NSRC: getattr(self.nat, NSRC)}
        two, nsrc = self.real[TWO], self.real[NSRC]

        def rec_two(srcs, relu, out=None):
            self.calls.append((TWO, [(int(c), int(u), int(bool(relu))) for _q, c, u in srcs]))
            return two(srcs, relu, out)

        def rec_n(srcs, out=None):
            self.calls.append((NSRC, [(int(c), int(u), int(bool(r))) for _q, c, u, r in srcs]))
            return nsrc(srcs, out)

        setattr(self.nat, TWO, rec_two)
        setattr(self.nat, NSRC, rec_n)
        return self

    def __exit__(self, *exc):
        for k, v in self.real.items():
            setattr(self.nat, k, v)


def rows(model):
    from common.quantity import resident
    return {n: tuple(getattr(p, f) for f in p.__slots__) for n, p in resident.describe(model).items()}


def check_net(nat, tag, device):
    """flatten=True on one of NETS: the plan, the summary, the launches and their operands, and the logits of plain = off = on on
    the example, on one image and on the flipped batch; then disable()."""
    from common.quantity import resident
    make, flattened, planned, launches, deferred = NETS[tag]
    net, x = make().to(device).eval(), cn.example().to(device)
    with torch.no_grad():
        plain = net(x)
    assert all(float(p.abs().max()) > 0 for p in _tuple(plain))
    with Recorder(nat) as rec:
        off = resident.enable(net, x, concat=True, avgpool=True)
        off_rows = rows(net)
        rec.calls[:] = []
        with torch.no_grad():
            assert same(net(x), plain)
        assert len(rec.calls) == planned and all(name == TWO for name, _ops in rec.calls), rec.calls
        on = resident.enable(net, x, concat=True, avgpool=True, flatten=True)          # verify=True
        d = resident.describe(net)
        assert on == dict(off, flattened_concats=flattened), (off, on)
        assert on["resident_concats"] == planned and d.flattened_concats == deferred, (on, d.flattened_concats)
        # the plans differ from the parent's in the `defer` of the deferred Concats and in nothing else
        on_rows = rows(net)
        slot = resident.Plan.__slots__.index("defer")
        for name, row in off_rows.items():
            want = row[:slot] + (True,) + row[slot + 1:] if name in deferred else row
            assert on_rows[name] == want, (name, on_rows[name], row)
        for shape_of in (lambda t: t, lambda t: t[:1], lambda t: torch.flip(t, dims=[0])):
            rec.calls[:] = []
            with torch.no_grad():
                assert same(net(shape_of(x)), tuple(shape_of(p) for p in _tuple(plain)))
            assert rec.calls == launches, rec.calls
        resident.disable(net)
        assert not resident.describe(net) and all("forward" not in m.__dict__ for m in net.modules())
        rec.calls[:] = []
        with torch.no_grad():
            assert same(net(x), plain)
        assert not rec.calls
    return on


# ---------------------------------------------------------------- the walker's classification (scripts/concat_geom_check.cpp)
KINDS = ("aligned16", "dword", "byte", "straddle")


def class_rows(lines):
    """{case argument: {kind: chunks of one pixel}} from the walker's "case ...: aligned16 A dword D byte B straddle S" lines."""
    rows = {}
    for line in lines:
        if line.startswith("case "):
            key, rest = line[5:].split(":")
            w = rest.split()
            rows[key] = dict(zip(w[0::2], (int(v) for v in w[1::2])))
    return rows


def check_paths_reached(rows):
    """Through the geometry header's own classification (cat_chunk_class): the case list reaches one 16-byte load, aligned
    dwords, byte-shifted dwords and chunks of two or more sources, each once without and once with an upsampled source; an
    aligned case holds 16-byte chunks only."""
    assert set(rows) == set(case_arg(c) for c in KERNEL_CASES)
    plain = [rows[case_arg(c)] for c in KERNEL_CASES if max(c[4]) == 1]
    ups = [rows[case_arg(c)] for c in KERNEL_CASES if max(c[4]) > 1]
    for name, group in (("plain", plain), ("upsampled", ups)):
        for kind in KINDS:
            assert any(r[kind] for r in group), (name, kind)
    for c in KERNEL_CASES:
        bases = np.cumsum([0] + list(c[3][:-1]))
        r = rows[case_arg(c)]
        assert sum(r.values()) == pad16(sum(c[3])) // 16
        if all(b % 16 == 0 for b in bases):
            assert r["dword"] == r["byte"] == r["straddle"] == 0, (c, r)
    assert rows[case_arg(GENERAL_CASES[2])] == dict(aligned16=0, dword=0, byte=0, straddle=2)      # eight sources, six in chunk 0
    assert rows[case_arg(GENERAL_CASES[1])]["straddle"] >= 1 and rows[case_arg(GENERAL_CASES[1])]["byte"] >= 1
