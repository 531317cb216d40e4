"""Shared by the tests of the windowed average pool over a NewAdd sum (test infrastructure, no product code): int16 sources for
the kernel's case list (avgpool_nets.KERNEL_CASES and its NumPy rule, which sums in int32 and so takes int16 as it stands), small
integer-simulation nets with a pool behind a sum built directly from NewConv2d info dicts -- no calibration, so the CPU suite (on
the doubles of tests/sum_pool_doubles.py) and the GPU suite build the same nets --, the float ResNet-D toy of golden G23 and the
random family RandomResNetD.  Module-level classes, so a planned net pickles.

Bits: an image at bit 5, activations at bit 4 unless a test says otherwise; the sum of two operands at bits gx, gy lies on the grid
g = max(0, gx, gy), and a convolution behind a pool reads at the bit of the pool's source, which is what the calibrator gives it.
"""
import random

import numpy as np
import torch
from torch import nn

import avgpool_nets as an
from avgpool_nets import pad16
from concat_nets import conv, example  # noqa: F401  (re-exported for the tests)

GRIDS = (0, 3, 8)
# b - g: both caps, the neighbours of zero and an odd one in between
RULE_SHIFTS = (-8, -3, -1, 0, 1, 8)
# more items (8 channels each) than 2048 x 256 lanes, so that the stride loop runs: 2 x 129 x 129 x 128 / 8 = 532 512 > 524 288, the
# smallest square plane at this batch and width (128 x 128 gives exactly 524 288: every lane one item)
STRIDE_LOOP_CASE = (2, 129, 129, 128, 3, 3, 1, 1, 1, 1)


def source16(rng, case, kind="random", g=0):
    """int16 NHWC source whose padding channels hold non-zero garbage.  kind "random": all of int16 with -32768 and 32767 planted;
    "grid": what a sum on grid g can hold, [-128 * 2^g, 127 * 2^g], both ends planted; "max" / "min": planes of 127 * 2^g /
    -128 * 2^g (saturation at positive shifts; |S| reaches 64 * 32768 at the cap with g = 8)."""
    N, H, W, C = case[:4]
    shape = (N, H, W, pad16(C))
    lo, hi = (-32768, 32767) if kind == "random" else (-128 << g, 127 << g)
    if kind in ("random", "grid"):
        a = rng.integers(lo, hi + 1, size=shape).astype(np.int16)
        a.flat[::7] = lo
        a.flat[3::11] = hi
        a[..., C:] = np.where(a[..., C:] == 0, 77, a[..., C:])
    else:
        a = np.full(shape, hi if kind == "max" else lo, np.int16)
        a[..., C:] = 77
    return a


def tie_source16(g):
    """avgpool_nets.tie_source scaled by 2^g: on the grid g the window means are k + 0.5 again at shift 0."""
    return (an.tie_source().astype(np.int16) << g).astype(np.int16)


# ---------------------------------------------------------------- a pool behind one sum
class SumPoolNet(nn.Module):
    """stem + ReLU -> NewAdd of two convolutions (+ ReLU) -> pool (+ ReLU) -> reader convolution(s), with what a test varies:
    pool        the nn.AvgPool2d (default: the 2x2 / 2 pool of the ResNet-D shortcut)
    relu_front  the ReLU between sum and pool (the add fuses it)
    relu_behind a ReLU behind the pool (the pool fuses it)
    read_bits   input bits of the readers (one or two convolutions read the pool)
    sum_bits    output bits of the add's two operands: the sum lies on the grid max(0, both)
    mode        "conv": nothing else; "concat" / "foreign": the pool's value goes to a Concat / a bare multiplication in front of
                the reader; "twice": the pool module is called a second time on another tensor."""

    def __init__(self, pool=None, relu_front=True, relu_behind=False, read_bits=(4,), sum_bits=(4, 4), mode="conv"):
        from common.quantity import Concat, NewAdd
        super(SumPoolNet, self).__init__()
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.a, self.b = conv(16, 16, 1, 4, sum_bits[0]), conv(16, 16, 3, 4, sum_bits[1], padding=1)
        self.add, self.radd = NewAdd(), nn.ReLU()
        self.pool = nn.AvgPool2d(2) if pool is None else pool
        self.r1 = nn.ReLU()
        self.c0 = conv(32 if mode == "concat" else 16, 8, 1, read_bits[0], 4)
        self.c1 = conv(16, 8, 3, read_bits[1], 4, padding=1) if len(read_bits) > 1 else None
        if mode == "concat":
            self.side, self.cat = conv(16, 16, 1, 4, read_bits[0], stride=2, seed=5), Concat()
        if mode == "twice":
            self.mid, self.rmid = conv(16, 16, 1, 4, 4, seed=3), nn.ReLU()
            self.c1 = conv(16, 8, 1, read_bits[0], 4, seed=1)
        self.relu_front, self.relu_behind, self.mode = relu_front, relu_behind, mode

    def forward(self, x):
        s = self.r0(self.stem(x))
        t = self.add(self.a(s), self.b(s))
        if self.relu_front:
            t = self.radd(t)
        p = self.pool(t)
        if self.relu_behind:
            p = self.r1(p)
        if self.mode == "concat":
            return self.c0(self.cat(p, self.side(s)))
        if self.mode == "foreign":
            return self.c0(p * 1.0)
        if self.mode == "twice":
            return self.c0(p), self.c1(self.pool(self.rmid(self.mid(s))))
        if self.c1 is not None:
            return self.c0(p), self.c1(p)
        return self.c0(p)


# ---------------------------------------------------------------- ResNet-D blocks
class _Block(nn.Module):
    """A bottleneck of NewConv2d layers: conv1 1x1 + ReLU, conv2 3x3 (stride) + ReLU, conv3 1x1, NewAdd with the shortcut, ReLU.
    `pool` (an nn.AvgPool2d or None) and `proj` (project the width) make the ResNet-D shortcut pool -> 1x1 convolution; without
    either the block input itself is the shortcut.  conv1 reads at `in_bit` and the projection at `proj_in_bit` (both default to
    `bit`, at which the inner layers work); conv3 and the projection write at `out_bit` / `proj_out_bit`."""

    def __init__(self, cin, mid, cout, stride=1, pool=None, proj=False, bit=4, in_bit=None, proj_in_bit=None, out_bit=None,
                 proj_out_bit=None, seed=0):
        from common.quantity import NewAdd
        super(_Block, self).__init__()
        in_bit = bit if in_bit is None else in_bit
        out_bit = bit if out_bit is None else out_bit
        self.conv1, self.relu1 = conv(cin, mid, 1, in_bit, bit, seed=seed), nn.ReLU()
        self.conv2, self.relu2 = conv(mid, mid, 3, bit, bit, stride=stride, padding=1, seed=seed), nn.ReLU()
        self.conv3 = conv(mid, cout, 1, bit, out_bit, seed=seed + 1)
        self.pool = pool
        self.proj = conv(cin, cout, 1, in_bit if proj_in_bit is None else proj_in_bit,
                         out_bit if proj_out_bit is None else proj_out_bit, seed=seed + 2) if proj else None
        self.add, self.relu3 = NewAdd(), nn.ReLU()

    def shortcut(self, x):
        if self.pool is not None:
            x = self.pool(x)
        return self.proj(x) if self.proj is not None else x

    def forward(self, x):
        y = self.conv3(self.relu2(self.conv2(self.relu1(self.conv1(x)))))
        return self.relu3(self.add(y, self.shortcut(x)))


class DBlockNet(nn.Module):
    """stem + ReLU -> front -> a ResNet-D block (`d`) -> head.
    front "identity": an identity bottleneck, whose sum the D block's conv1 and pool read;
          "tail":     two identity bottlenecks at widths fq_block_tail_i8 takes (128 channels, 64 inside): the second add runs its
                      conv3 and the D block's conv1 in one launch, and the pool reads the wide tensor that launch wrote;
          "proj":     an identity bottleneck at 64 channels and a D block with 64 channels inside and 128 out: the widths at which
                      fq_block_tail_proj_i8 takes conv3 + add + projection, the projection's operand being the POOLED tensor at
                      stride 1;
    skip  the D block keeps the plane (3x3 / 1 / 1 pool, stride 1) and a further add reads the front's sum as well: pool, conv1
          and that add are its three readers."""

    def __init__(self, front="identity", skip=False, pool=None):
        from common.quantity import NewAdd
        super(DBlockNet, self).__init__()
        w, mid = {"identity": (16, 16), "tail": (128, 64), "proj": (64, 64)}[front]
        self.stem, self.r0 = conv(3, w, 3, 5, 4, padding=1), nn.ReLU()
        self.f1 = _Block(w, mid, w, seed=1)
        self.f2 = _Block(w, mid, w, seed=2) if front == "tail" else None
        if pool is None:
            pool = nn.AvgPool2d(3, 1, 1) if skip else nn.AvgPool2d(2, 2)
        self.d = _Block(w, mid, w if skip else 2 * w, stride=1 if skip else 2, pool=pool, proj=True, seed=3)
        if skip:
            self.side, self.add2, self.r2 = conv(w, w, 1, 4, 4, seed=7), NewAdd(), nn.ReLU()
        self.head = conv(w if skip else 2 * w, 8, 1, 4, 4)
        self.skip = skip

    def forward(self, x):
        t = self.f1(self.r0(self.stem(x)))
        if self.f2 is not None:
            t = self.f2(t)
        u = self.d(t)
        if self.skip:
            u = self.r2(self.add2(self.side(u), t))
        return self.head(u)


# ---------------------------------------------------------------- golden G23
class _FloatBottleneckD(nn.Module):
    def __init__(self, cin, mid, cout, stride=1):
        from common.quantity import Eltwise
        super(_FloatBottleneckD, self).__init__()
        self.conv1, self.relu1 = nn.Conv2d(cin, mid, 1), nn.ReLU(False)
        self.conv2, self.relu2 = nn.Conv2d(mid, mid, 3, stride=stride, padding=1), nn.ReLU(False)
        self.conv3 = nn.Conv2d(mid, cout, 1)
        short = []
        if stride != 1:
            short.append(nn.AvgPool2d(2, 2))
        if stride != 1 or cin != cout:
            short.append(nn.Conv2d(cin, cout, 1))
        self.downsample = nn.Sequential(*short)
        self.Eltwise = Eltwise()
        self.relu3 = nn.ReLU(False)

    def forward(self, x):
        y = self.conv3(self.relu2(self.conv2(self.relu1(self.conv1(x)))))
        return self.relu3(self.Eltwise(y, self.downsample(x)))


class G23Net(nn.Module):
    """The FLOAT net calibrated for golden G23 (tests/golden/make_golden_resnetd.py): a 3-stage toy ResNet-D -- stem, one identity
    bottleneck, two downsampling bottlenecks whose shortcut is AvgPool2d(2, 2) -> 1x1 convolution reading ReLU(Eltwise), global
    pool, View, Linear.  Input 3 x 12 x 12, widths 8 to 32.  The marker layers come from whichever `common.quantity` is imported:
    the reference's when the golden is captured, the product's in the tests."""

    def __init__(self):
        from common.quantity import View
        super(G23Net, self).__init__()
        self.stem, self.relu0 = nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(False)
        self.block1 = _FloatBottleneckD(8, 8, 8)
        self.block2 = _FloatBottleneckD(8, 8, 16, stride=2)
        self.block3 = _FloatBottleneckD(16, 16, 32, stride=2)
        self.pool_g = nn.AvgPool2d(3)
        self.view = View()
        self.fc = nn.Linear(32, 5)

    def forward(self, x):
        x = self.block3(self.block2(self.block1(self.relu0(self.stem(x)))))
        return self.fc(self.view(self.pool_g(x)))


def g23_net():
    return G23Net()


G23_SHAPE = (4, 3, 12, 12)
G23_SEED, G23_CALIB_SEED, G23_INPUT_SEED = 23, 2300, 2323


# ---------------------------------------------------------------- the random family
def _near(rng, bit, spread, lo=2, hi=6):
    return min(hi, max(lo, bit + rng.randint(-spread, spread)))


class RandomResNetD(nn.Module):
    """A random ResNet-D-shaped integer-simulation net drawn from `seed`: plane 8 or 16, widths 8 to 64, 2 to 4 blocks behind the
    stem.  The first block is an identity bottleneck and the second a D block, so every model has at least one windowed pool over
    a sum; every later block is a D block (while the plane allows) or an identity one.  A D block's pool is 2x2 / 2 or 3x3 / 2 / 1
    with either count_include_pad.  Bits: conv3 and the projection of a block write at bits drawn from 2 .. 6, so the sum's grid
    g lies there too; the next block's conv1 reads within 1 of conv3's bit and its projection -- the pool's reader -- within 2 of
    that, clipped to 0 .. 8.  So |b - g| <= 8 always holds and a pool with one reader is in the class the rule admits.  One pool in
    eight gets a second reader at ANOTHER bit (an extra output of the model): readers at two bits, which the rule declines.
    `pools`: [(module name, admitted)]."""

    def __init__(self, seed):
        super(RandomResNetD, self).__init__()
        rng = random.Random(seed)
        self.plane = rng.choice((8, 16))
        width = rng.choice((8, 16, 24))
        cur = rng.randint(2, 6)                             # the bit the value in front of the next block was written at
        self.stem, self.r0 = conv(3, width, 3, 5, cur, padding=1, seed=seed), nn.ReLU()
        blocks, plane, self.pools, aux = [], self.plane, [], {}
        for i in range(rng.randint(2, 4)):
            down = i == 1 or (i > 1 and plane >= 4 and rng.random() < 0.6)
            mid = rng.choice((8, 16))
            in_bit = cur if i == 0 else _near(rng, cur, 1)
            out_bit = rng.randint(2, 6)
            if i == 0 or not down:
                cout = width if rng.random() < 0.7 else min(64, width + 8)     # (a width change: a projection without a pool)
                blk = _Block(width, mid, cout, proj=cout != width, in_bit=in_bit, out_bit=out_bit,
                             proj_out_bit=_near(rng, out_bit, 1), seed=seed + i)
            else:
                pool = (nn.AvgPool2d(2, 2, count_include_pad=rng.random() < 0.5) if rng.random() < 0.5 else
                        nn.AvgPool2d(3, 2, 1, count_include_pad=rng.random() < 0.5))
                cout = min(64, rng.choice((width, 2 * width)))
                pb = _near(rng, in_bit, 2, 0, 8)
                blk = _Block(width, mid, cout, stride=2, pool=pool, proj=True, in_bit=in_bit, proj_in_bit=pb, out_bit=out_bit,
                             proj_out_bit=_near(rng, out_bit, 1), seed=seed + i)
                plane //= 2
                admitted = True
                if rng.random() < 0.125:
                    aux[str(i)] = conv(width, 8, 1, pb + (1 if pb < 8 else -1), 4, seed=seed + 50 + i)
                    admitted = False
                self.pools.append(("blocks.%d.pool" % i, admitted))
            blocks.append(blk)
            width, cur = cout, out_bit
        self.blocks = nn.ModuleList(blocks)
        self.aux = nn.ModuleDict(aux)
        self.head = conv(width, 8, 1, cur, 4, seed=seed + 99)

    def example(self, seed=1):
        return torch.randn(4, 3, self.plane, self.plane, generator=torch.Generator().manual_seed(seed))

    def forward(self, x):
        x = self.r0(self.stem(x))
        extra = []
        for i, blk in enumerate(self.blocks):
            if str(i) in self.aux:
                # the block's own forward with the pooled value read a second time
                y = blk.conv3(blk.relu2(blk.conv2(blk.relu1(blk.conv1(x)))))
                p = blk.pool(x)
                extra.append(self.aux[str(i)](p))
                x = blk.relu3(blk.add(y, blk.proj(p)))
            else:
                x = blk(x)
        out = self.head(x)
        return (out,) + tuple(extra) if extra else out
