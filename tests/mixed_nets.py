"""Random graphs that mix every layer type a switch of resident.enable() takes (test infrastructure, no product code; DESIGN
section 27): the generator of tests/test_mixed_plan_cpu.py, tests/test_gpu_mixed_fuzz.py and scripts/recon_fuzz.py's `mixed` mode.

  RandomMixedNet(index, seed)   a 3x3 stem, two to six random steps and the head (whole-plane pool, View, Linear) on 8 or 16 pixels
                                at batch 4, widths 8 to 64.  `plan` is the list of calls ("call", module name, [input names], output
                                name) that forward() walks, as cases.RandomNet; `steps` names the step kinds drawn.  Imports under
                                the REFERENCE's `common` package too (the golden script): Eltwise / Concat / View come from whichever
                                `common.quantity` is imported, Slice from shuffle_nets.
  family()                      the (index, seed) pairs of the fixed family both tests run.
  ALL_SWITCHES                  the eight switches, all on.
  facts(net, plans)             what the coverage conditions count, from describe(net) and the recorded calls.
  perturbed(info, index)        a seeded change of output_bit (with bias_bit) on up to three layers and, where a table activation
                                has two convolution readers, of the input_bit of one of them.

The steps (one is drawn per position; `act` is an nn.ReLU, an nn.ReLU6, a listed table activation or nothing, now and then in place):
  dense     1x1 / 3x3 / 5x5 convolution, stride 1 or 2, act        sep       depthwise 3x3 / 5x5 (stride 1 / 2), act, 1x1, act
  grouped   grouped 1x1 / 3x3 (4 to 64 channels per group), act    res       1x1 -> depthwise / grouped / dense 3x3 -> 1x1, added to
  opres     a depthwise / grouped layer or a Slice straight into             its input, a shuffle of it, or a 1x1 projection of it
            an Eltwise                                             cat2      two convolutions joined
  incept    1x1 | 1x1 -> 3x3 | AvgPool -> 1x1 | MaxPool -> 1x1 and up to five more leaves, one of them upsampled by 2 or 4, nested
            as a chain, a tree or with a ReLU behind an inner Concat (3 to 9 leaves)
  fpn       a stride-2 convolution, upsampled and joined with a lateral 1x1
  unit      ShuffleNet unit, stride 1 (Slice | Slice -> branch, Concat, shuffle) or stride 2
  chan      a Slice or a shuffle alone                            pool      windowed AvgPool2d (3x3 s1, 2x2 s2) or MaxPool2d behind
  actmove   a table activation that reaches its convolution               the value, a Slice, a shuffle or a Concat of it
            through a max-pool, Slice, shuffle, upsampling or nested Concat
and what the planner has to leave alone:
  sumread   a NewAdd sum read by a shuffle, a Slice, a table activation or a windowed pool
  actread   a table activation read by a windowed average pool or by an Eltwise
  twice     a shuffle, a table activation or an nn.ReLU6 module called twice
  revoke    a table activation joined with a NewAdd sum or a windowed pool's output by a Concat (the first plan takes it, the lossy
            verification takes it back), next to a nested Concat
"""
import random

import numpy as np
import torch
from torch import nn

import common.quantity as _cq
from activation_nets import ACTIVATIONS
from shuffle_nets import Slice

Eltwise, Concat, View = _cq.Eltwise, _cq.Concat, _cq.View

ALL_SWITCHES = dict(depthwise=True, concat=True, avgpool=True, grouped=True, relu6=True, flatten=True, shuffle=True, activations=True)
TABLE_NAMES = [n for n in ACTIVATIONS if n != "PReLU"]      # (a module with a weight does not go through the calibration flow)
STEPS = ("dense", "sep", "grouped", "res", "opres", "cat2", "incept", "incept", "fpn", "unit", "chan", "pool", "actmove", "actmove",
         "sumread", "sumread", "actread", "twice", "revoke")
WIDTHS = (8, 12, 16, 20, 24, 32, 40, 48, 58, 64)
FAMILY_SEED, FAMILY_SIZE = 18, 40


def family():
    return [(i, FAMILY_SEED) for i in range(FAMILY_SIZE)]


def _group_counts(c):
    return [g for g in (2, 3, 4, 5, 6, 8, 10, 12, 16) if g < c and c % g == 0 and 4 <= c // g <= 64 and (c // g) % 4 == 0]


def _divisors(c):
    return [g for g in range(2, c + 1) if c % g == 0]


class RandomMixedNet(nn.Module):

    def __init__(self, index, seed):
        super(RandomMixedNet, self).__init__()
        rng = random.Random(seed * 100003 + index * 31 + 7)
        self.cin, self.batch = 3, 4
        self.size = rng.choice((8, 16))
        self.plan, self.steps, self.count = [], [], 0
        self.has_bn = rng.random() < 0.2
        ch, hw = {"x": 3}, {"x": self.size}

        def add(module):
            name = "m%d" % self.count
            self.count += 1
            setattr(self, name, module)
            return name

        def call(m, ins, c, s):
            out = "t%d" % len(self.plan)
            self.plan.append(("call", m, list(ins), out))
            ch[out], hw[out] = c, s
            return out

        def conv(src, cout, k=1, s=1, groups=1):
            if hw[src] < 4:
                s = 1
            bn = self.has_bn and groups == 1 and rng.random() < 0.5
            out = call(add(nn.Conv2d(ch[src], cout, k, s, k // 2, groups=groups, bias=not (bn and rng.random() < 0.5))), [src], cout,
                       (hw[src] + 2 * (k // 2) - k) // s + 1)
            if bn:                                            # (registered right behind its convolution, as merge_bn pairs them)
                out = call(add(nn.BatchNorm2d(cout)), [out], cout, hw[out])
            return out

        def one(module, src, c=None, s=None):
            return call(add(module), [src], ch[src] if c is None else c, hw[src] if s is None else s)

        def table(src, inplace_ok=True):
            m = ACTIVATIONS[rng.choice(TABLE_NAMES)]()
            if inplace_ok and hasattr(m, "inplace") and rng.random() < 0.2:
                m.inplace = True
            return one(m, src)

        def act(src, kinds=("relu", "relu", "relu6", "relu6", "table", "table", "none")):
            kind = rng.choice(kinds)
            if kind == "none":
                return src
            if kind == "table":
                return table(src)
            return one(nn.ReLU(rng.random() < 0.1) if kind == "relu" else nn.ReLU6(rng.random() < 0.1), src)

        def relu(src):
            return one(nn.ReLU(False), src)

        def join(a, b):
            return call(add(Concat()), [a, b], ch[a] + ch[b], hw[a])

        def plus(a, b):
            return call(add(Eltwise()), [a, b], ch[a], hw[a])

        def dw(src, k=None, s=1):
            return conv(src, ch[src], k or rng.choice((3, 5)), s, groups=ch[src])

        def grouped(src, k=None, s=1, cout=None):
            """a grouped layer on `src` (behind a 1x1 to a width that splits, if its own does not) -> its output"""
            if not _group_counts(ch[src]):
                src = relu(conv(src, rng.choice((16, 24, 32, 48, 64))))
            g = rng.choice(_group_counts(ch[src]))
            if cout is None:
                cout = g * rng.choice([w for w in (4, 8, 12, 16) if g * w <= 96])
            return conv(src, cout, k or rng.choice((1, 3)), s, groups=g)

        def up(src, s):
            return one(nn.UpsamplingNearest2d(scale_factor=s), src, None, hw[src] * s)

        def narrow(src):
            """back to at most 64 channels"""
            return act(conv(src, rng.choice((16, 24, 32))), ("relu", "relu6", "table")) if ch[src] > 64 else src

        def mover(src):
            """one op that Quantity commutes with behind `src`"""
            kind = rng.choice(("maxpool", "slice", "shuffle", "up", "nest"))
            c = ch[src]
            if kind == "maxpool" and hw[src] >= 4:
                k, s, p = rng.choice(((2, 2, 0), (3, 1, 1), (3, 2, 1)))
                return one(nn.MaxPool2d(k, s, p), src, None, (hw[src] + 2 * p - k) // s + 1)
            if kind == "slice" or (kind == "up" and hw[src] > 8):
                a = rng.randint(0, c - 2)
                b = rng.randint(a + 1, c)
                return one(Slice(a, b), src, b - a)
            if kind == "up":
                return up(src, rng.choice((2, 2, 4)) if hw[src] <= 4 else 2)
            if kind == "nest":
                a, b = rng.randint(1, c - 1), rng.randint(1, c - 1)
                return join(join(one(Slice(0, a), src, a), one(Slice(b, c), src, c - b)), one(Slice(0, b), src, b))
            return one(nn.ChannelShuffle(rng.choice(_divisors(c))), src)

        cur = act(conv("x", rng.choice((8, 12, 16, 24, 32)), 3, rng.choice((1, 1, 2)) if self.size == 16 else 1), ("relu", "relu", "relu6", "table"))
        for _ in range(rng.randint(2, 6)):
            kind = rng.choice(STEPS)
            c = ch[cur]
            if kind == "fpn" and (hw[cur] < 4 or hw[cur] % 2):
                kind = "dense"
            self.steps.append(kind)
            if kind == "dense":
                cur = act(conv(cur, rng.choice(WIDTHS), rng.choice((1, 1, 3, 3, 5)), rng.choice((1, 1, 2))))
            elif kind == "sep":
                cur = act(conv(act(dw(cur, s=rng.choice((1, 1, 2)))), rng.choice(WIDTHS)))
            elif kind == "grouped":
                cur = act(grouped(cur, s=rng.choice((1, 1, 2))))
            elif kind == "res":
                mid = rng.choice((8, 16, 24, 32))
                y = act(conv(cur, mid), ("relu", "relu6", "table"))
                inner = rng.choice(("dw", "grouped", "dense"))
                s = rng.choice((1, 2)) if hw[cur] >= 4 and hw[cur] % 2 == 0 and rng.random() < 0.35 else 1
                y = dw(y, s=s) if inner == "dw" else grouped(y, 3, s) if inner == "grouped" else conv(y, mid, 3, s)
                y = conv(act(y, ("relu", "relu6", "none")), c)
                short = conv(cur, c, 1, s) if s == 2 or rng.random() < 0.3 else cur
                if short is cur and rng.random() < 0.25:
                    short = one(nn.ChannelShuffle(rng.choice(_divisors(c))), cur)
                cur = plus(y, short) if rng.random() < 0.7 else plus(short, y)
                cur = act(cur, ("relu", "relu", "relu", "none", "relu6", "table"))
            elif kind == "opres":
                how = rng.choice(("dw", "grouped", "slice"))
                if how == "dw":
                    y = dw(cur)
                elif how == "grouped":
                    if not _group_counts(c):
                        cur = relu(conv(cur, rng.choice((16, 24, 32, 48))))
                        c = ch[cur]
                    y = grouped(cur, cout=c)
                else:
                    wide = act(conv(cur, 2 * c if 2 * c <= 96 else c + 8, rng.choice((1, 3))), ("relu", "relu6", "none"))
                    a = rng.randint(0, ch[wide] - c)
                    y = one(Slice(a, a + c), wide, c)
                cur = act(plus(y, cur), ("relu", "relu", "none"))
            elif kind == "cat2":
                a = act(conv(cur, rng.choice((8, 12, 20, 32)), 3), ("none", "none", "relu6", "relu"))
                b = act(conv(cur, rng.choice((4, 12, 16, 26)), 1), ("none", "none", "relu6", "relu"))
                cur = act(join(a, b), ("relu", "relu", "none", "relu6"))
            elif kind == "incept":
                w = lambda: rng.choice((4, 8, 12, 16, 20))     # noqa: E731
                leaf_act = ("relu", "relu", "relu6", "relu6", "none")
                leaves = [act(conv(cur, w()), leaf_act),
                          act(conv(act(conv(cur, w()), ("relu", "relu6", "table")), w(), 3), leaf_act),
                          act(conv(one(nn.AvgPool2d(3, 1, 1), cur), w()), leaf_act),
                          act(conv(one(nn.MaxPool2d(3, 1, 1), cur), w()), leaf_act)]
                rng.shuffle(leaves)
                leaves = leaves[:rng.randint(2, 4)]
                if hw[cur] >= 4 and hw[cur] % 4 == 0 and rng.random() < 0.7:      # an upsampled leaf
                    f = rng.choice((2, 2, 4))
                    if hw[cur] < 8:                            # (a plane of 4 pixels halves once)
                        f = 2
                    small = cur
                    for _s in range(f // 2):
                        small = act(conv(small, w(), 3, 2), ("relu", "relu6")) if rng.random() < 0.6 else one(nn.MaxPool2d(2), small, None, hw[small] // 2)
                    leaves.insert(rng.randint(0, len(leaves)), up(act(conv(small, w()), leaf_act), f))
                for _e in range(rng.choice((0, 0, 1, 2, 5))):
                    leaves.append(act(conv(cur, w(), rng.choice((1, 3))), leaf_act))
                leaves = leaves[:9]
                shape = rng.choice(("chain", "tree", "relu_inside"))
                if shape == "tree" and len(leaves) >= 4:
                    half = len(leaves) // 2
                    left, right = leaves[0], leaves[half]
                    for t in leaves[1:half]:
                        left = join(left, t)
                    for t in leaves[half + 1:]:
                        right = join(right, t)
                    cur = join(left, right)
                else:
                    cur = leaves[0]
                    for n, t in enumerate(leaves[1:]):
                        cur = join(cur, t)
                        if shape == "relu_inside" and n == 0 and len(leaves) > 2:
                            cur = relu(cur)
                cur = act(cur, ("relu", "none", "none"))
            elif kind == "fpn":
                lateral = act(conv(cur, rng.choice((8, 12, 16))), ("none", "relu", "relu6"))
                down = act(conv(cur, rng.choice((8, 16, 20)), 3, 2), ("relu", "relu6", "table"))
                top = act(conv(down, rng.choice((8, 12, 24)), rng.choice((1, 3))), ("none", "relu", "relu6"))
                cur = join(up(top, 2), lateral) if rng.random() < 0.5 else join(lateral, up(top, 2))
            elif kind == "unit":
                g = rng.choice(_divisors(c))
                if hw[cur] >= 4 and hw[cur] % 2 == 0 and rng.random() < 0.3:
                    half = rng.choice((6, 10, 16, 29))
                    a = act(conv(dw(cur, 3, 2), half), ("relu", "relu6"))
                    b = act(conv(dw(act(conv(cur, half), ("relu", "relu6", "table")), 3, 2), half), ("relu", "relu6"))
                    cur = one(nn.ChannelShuffle(rng.choice(_divisors(2 * half))), join(a, b))
                else:
                    cut = rng.randint(1, c - 1)
                    left, right = one(Slice(0, cut), cur, cut), one(Slice(cut, c), cur, c - cut)
                    r = c - cut
                    b = act(conv(dw(act(conv(right, r), ("relu", "relu6", "table")), 3, 1), r), ("relu", "relu6"))
                    cur = one(nn.ChannelShuffle(g), join(left, b))
            elif kind == "chan":
                if rng.random() < 0.5:
                    cur = one(nn.ChannelShuffle(rng.choice(_divisors(c))), cur)
                else:
                    a = rng.randint(0, c - 4)
                    b = rng.randint(a + 4, c)
                    cur = one(Slice(a, b), cur, b - a)
                cur = act(conv(cur, rng.choice(WIDTHS), rng.choice((1, 3))))
            elif kind == "pool":
                front = rng.choice(("none", "slice", "shuffle", "cat"))
                if front == "slice":
                    a = rng.randint(0, c - 4)
                    b = rng.randint(a + 4, c)
                    cur = one(Slice(a, b), cur, b - a)
                elif front == "shuffle":
                    cur = one(nn.ChannelShuffle(rng.choice(_divisors(c))), cur)
                elif front == "cat":
                    cur = join(act(conv(cur, rng.choice((8, 12, 20))), ("relu", "none")), act(conv(cur, rng.choice((4, 12, 16)), 3), ("relu", "none")))
                which = rng.choice(("avg3", "avg3", "avg2", "avg2", "max"))
                if which == "avg2" and (hw[cur] < 4 or hw[cur] % 2):
                    which = "avg3"
                if which == "avg3":
                    cur = one(nn.AvgPool2d(3, 1, 1, count_include_pad=rng.random() < 0.5), cur)
                elif which == "avg2":
                    cur = one(nn.AvgPool2d(2, 2), cur, None, hw[cur] // 2)
                else:
                    cur = one(nn.MaxPool2d(3, 1, 1), cur)
                cur = act(conv(cur, rng.choice(WIDTHS), rng.choice((1, 3))))
            elif kind == "actmove":
                src = rng.choice(("dense", "dw", "grouped"))
                y = conv(cur, rng.choice(WIDTHS[:8]), rng.choice((1, 3))) if src == "dense" else dw(cur) if src == "dw" else grouped(cur)
                y = table(y, inplace_ok=False)
                for _m in range(rng.randint(0, 2)):
                    y = mover(y)
                cur = act(conv(y, rng.choice(WIDTHS), rng.choice((1, 3))))
            elif kind == "sumread":
                s = plus(conv(cur, c, rng.choice((1, 3))), cur)
                reader = rng.choice(("shuffle", "slice", "table", "table", "avg3", "avg2"))
                if reader == "avg2" and (hw[cur] < 4 or hw[cur] % 2):
                    reader = "avg3"
                if reader == "shuffle":
                    s = one(nn.ChannelShuffle(rng.choice(_divisors(c))), s)
                elif reader == "slice":
                    a = rng.randint(0, c - 4)
                    b = rng.randint(a + 4, c)
                    s = one(Slice(a, b), s, b - a)
                elif reader == "table":
                    s = table(s)
                else:
                    s = one(nn.AvgPool2d(3, 1, 1), s) if reader == "avg3" else one(nn.AvgPool2d(2, 2), s, None, hw[s] // 2)
                cur = act(conv(s, rng.choice(WIDTHS)))
            elif kind == "actread":
                a = table(conv(cur, c, rng.choice((1, 3))), inplace_ok=False)
                if rng.random() < 0.5:
                    cur = one(nn.AvgPool2d(3, 1, 1), a)
                else:
                    cur = plus(a, cur)
                cur = act(conv(cur, rng.choice(WIDTHS)))
            elif kind == "twice":
                what = rng.choice(("shuffle", "table", "relu6"))
                if what == "relu6":
                    m = add(nn.ReLU6(False))
                    y = call(m, [conv(cur, c, 3)], c, hw[cur])
                    cur = call(m, [conv(y, c)], c, hw[y])
                else:
                    y = conv(cur, c) if what == "table" else cur
                    m = add(ACTIVATIONS[rng.choice(TABLE_NAMES)]() if what == "table" else nn.ChannelShuffle(rng.choice(_divisors(c))))
                    y = call(m, [y], c, hw[y])
                    y = call(m, [y], c, hw[y])
                    cur = act(conv(y, rng.choice(WIDTHS)))
            else:
                assert kind == "revoke"
                b1, b2, b3 = relu(conv(cur, 8)), relu(conv(cur, 12, 3)), relu(conv(cur, 8))
                nest = relu(conv(join(join(b1, b2), b3), c))
                a = table(conv(nest, rng.choice((8, 12, 16)), rng.choice((1, 3))), inplace_ok=False)
                other = plus(conv(nest, c), nest) if rng.random() < 0.5 else one(nn.AvgPool2d(3, 1, 1), nest)
                cur = act(conv(join(a, other), rng.choice(WIDTHS)))
            cur = narrow(cur)
        cur = one(nn.ReLU(False), conv(cur, 16))
        cur = one(nn.AvgPool2d(hw[cur]), cur, None, 1)
        self.plan.append(("call", add(nn.Linear(16, 10)), [one(View(), cur)], "y"))
        self.n = len(list(self.modules()))
        gen = torch.Generator().manual_seed(1000 * seed + index)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if p.dim() > 1:
                    p.copy_(torch.randn(p.shape, generator=gen) * (1.5 / max(1, p[0].numel()) ** 0.5))
                else:
                    p.copy_(torch.randn(p.shape, generator=gen) * 0.2)
            for m in self.modules():                          # (statistics and affine terms that are not the identity)
                if isinstance(m, nn.BatchNorm2d):
                    m.weight.copy_(0.6 + 0.8 * torch.rand(m.weight.shape, generator=gen))
                    m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=gen))
                    m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))

    def forward(self, x):
        t = {"x": x}
        for _op, m, ins, out in self.plan:
            t[out] = getattr(self, m)(*[t[i] for i in ins])
        return t["y"]


def batches(model, index, seed, n=3):
    """n seeded (images, labels) pairs on the host for model `index`: the test input first, the calibration batches behind it."""
    g = np.random.default_rng(77000 + 1009 * seed + index)
    shape = (model.batch, model.cin, model.size, model.size)
    return [(torch.from_numpy(g.standard_normal(shape, dtype=np.float32)), torch.zeros(shape[0], dtype=torch.long)) for _ in range(n)]


# ---------------------------------------------------------------- what the tests count on a planned model
class Graph(object):
    """The recorded calls of a (rebuilt) RandomMixedNet: who made each tensor and who reads it."""

    def __init__(self, net):
        self.net = net
        self.made_by = {}                                     # tensor name -> (module name, [input names])
        self.readers = {}                                     # tensor name -> [module name]
        self.reads = {}                                       # tensor name -> [(module name, the output of that call)]
        self.calls = {}                                       # module name -> number of calls
        for _op, m, ins, out in net.plan:
            self.made_by[out] = (m, ins)
            self.calls[m] = self.calls.get(m, 0) + 1
            for t in ins:
                self.readers.setdefault(t, []).append(m)
                self.reads.setdefault(t, []).append((m, out))

    def module(self, name):
        return getattr(self.net, name)

    def kind(self, name):
        m = self.module(name)
        t = type(m).__name__
        if t == "NewConv2d":
            k = m.Conv
            return "dense" if k.groups == 1 else "depthwise" if k.groups == k.in_channels == k.out_channels else "grouped"
        if isinstance(m, nn.AvgPool2d):
            return "avgpool"
        if isinstance(m, nn.Upsample):
            return "upsample"
        if isinstance(m, nn.ReLU6):
            return "relu6"
        if isinstance(m, (nn.BatchNorm2d, nn.Identity)) or t in ("Identity", "EmptyLayer"):
            return "identity"
        return {"NewAdd": "add", "NewLinear": "linear", "Concat": "concat", "Slice": "slice", "ChannelShuffle": "shuffle",
                "MaxPool2d": "maxpool", "ReLU": "relu", "View": "view"}.get(t, "act" if t in ACTIVATIONS else t)

    def maker(self, t, through=("relu", "relu6", "identity")):
        """The module that made tensor t, looking through clamps (and folded BatchNorms): (module name, its inputs, the clamps)."""
        seen = []
        while t in self.made_by and self.kind(self.made_by[t][0]) in through:
            seen.append(self.made_by[t][0])
            t = self.made_by[t][1][0]
        name, ins = self.made_by.get(t, (None, []))
        return name, ins, seen

    def out_of(self, name):
        return [out for _op, m, _ins, out in self.net.plan if m == name]

    def final_readers(self, t, plans):
        """The modules that read tensor t, looking through a fused clamp / a folded BatchNorm behind it."""
        out = []
        for r, o in self.reads.get(t, []):
            k = self.kind(r)
            if k == "identity" or (k in ("relu", "relu6") and "forward" in self.module(r).__dict__):
                out.extend(self.final_readers(o, plans))
            else:
                out.append(r)
        return out


def _leaves(g, plans, name):
    """[(maker name, clamps, upsampling module or None)] of the launch of planned Concat `name`, deferred operands expanded."""
    out = []
    for t in g.made_by[g.out_of(name)[0]][1]:
        m, ins, clamps = g.maker(t)
        if m is not None and g.kind(m) == "concat" and m in plans and plans[m].defer:
            out.extend(_leaves(g, plans, m))
        elif m is not None and g.kind(m) == "upsample" and m in plans and plans[m].defer:
            src, _i, c2 = g.maker(ins[0])
            out.append((src, c2, m))
        else:
            out.append((m, clamps, None))
    return out


def facts(net, plans):
    """Counts of the interactions (a) to (g) of the coverage conditions on one planned model (plans = resident.describe(net)), and
    the two properties of the accounting that need the graph: `pool_operand` (a planned windowed pool whose value a Concat or an
    add reads) and `fp32_reader` ((producer, reader) where the producer emits no fp32 and the reader has no integer path)."""
    g = Graph(net)
    f = dict.fromkeys(("a", "b", "c", "d", "e", "f", "sum_shuffle", "sum_act", "sum_pool", "act_avgpool", "act_add", "act_two_bits",
                       "twice", "inplace", "cat_two_grids"), 0)
    f["pool_operand"], f["fp32_reader"] = [], []
    flattened = set(plans.flattened_concats)
    for name, p in plans.items():
        k = g.kind(name)
        outs = g.out_of(name)
        if k == "act" and p.table is not None:
            src, _ins, _cl = g.maker(g.made_by[outs[0]][1][0], through=("identity",))
            f["a"] += g.kind(src) in ("depthwise", "grouped")
            rd = [r for r in g.final_readers(outs[0], plans) if r in plans]
            f["b"] += any(g.kind(r) in ("maxpool", "slice", "shuffle", "upsample") or (g.kind(r) == "concat" and r in flattened) for r in rd)
        if k == "concat" and not p.defer:
            lv = _leaves(g, plans, name)
            clipped = any(m in plans and plans[m].clip for m, _cl, _u in lv)
            f["c"] += len(lv) >= 3 and clipped and any(u is not None for _m, _cl, u in lv)
        if k == "avgpool":
            src, _ins, _cl = g.maker(g.made_by[outs[0]][1][0])
            f["d"] += g.kind(src) in ("slice", "shuffle", "concat")
            f["pool_operand"] += [r for r in g.final_readers(outs[0], plans) if g.kind(r) in ("concat", "add")]
        if k == "add" and p.resident_add:
            srcs = [g.maker(t, through=("identity",))[0] for t in g.made_by[outs[0]][1]]
            f["e"] += any(s in plans and g.kind(s) in ("depthwise", "grouped", "slice") and (g.kind(s) == "slice" or plans[s].depthwise or plans[s].grouped)
                          for s in srcs)
        if not p.emit_f32:
            for o in outs:
                if o == "y":
                    f["fp32_reader"].append((name, "the model's output"))
                for r in g.final_readers(o, plans):
                    m, kr = g.module(r), g.kind(r)
                    reads_int = r in plans or "forward" in m.__dict__ or kr == "linear" or (
                        kr == "dense" and m._int8_ok(m.Conv) and not m._stem_fold(m.Conv))
                    if not reads_int:
                        f["fp32_reader"].append((name, r))
    f["f"] = int(bool(plans.activations_revoked) and bool(flattened))
    for why in plans.shuffle_left.values():
        f["sum_shuffle"] += "NewAdd sum" in why
        f["twice"] += "more than once" in why
    for why in plans.activations_left.values():
        f["sum_act"] += "NewAdd sum" in why
        f["act_avgpool"] += "the average pool" in why
        f["act_add"] += "the NewAdd" in why
        f["act_two_bits"] += "different bits" in why
        f["twice"] += "more than once" in why
        f["inplace"] += "inplace=True" in why
    for why in plans.relu6_left.values():
        f["twice"] += "more than once" in why
    for name in g.calls:
        k = g.kind(name)
        if name in plans:
            continue
        ins = g.made_by[g.out_of(name)[0]][1]
        if k == "avgpool" and g.kind(g.readers[g.out_of(name)[0]][0]) != "view":
            src = g.maker(ins[0])[0]
            f["sum_pool"] += src in plans and plans[src].resident_add
        if k == "concat":
            ops = [g.maker(t)[0] for t in ins]
            if all(o in plans and not plans[o].resident_add and plans[o].narrow_bit is not None and g.kind(o) != "avgpool" for o in ops):
                f["cat_two_grids"] += plans[ops[0]].narrow_bit != plans[ops[1]].narrow_bit
    return f


def perturbed(info, index, net=None):
    """`info` (Reconstruction.get_quantity_information) with a seeded change of output_bit, and bias_bit with it, on up to three
    convolutions -- operands on two grids, output_bit <= -2 under a ReLU6, shifts outside [1, 16] -- and, where the model has a
    table activation with two convolution readers, another input_bit for one of the two (readers at two bits)."""
    rng = random.Random(4049 * index + 11)
    out = type(info)((k, dict(v)) for k, v in info.items())
    convs = [k for k, v in out.items() if v.get("layer_type") == "Conv2d"]
    for name in rng.sample(convs, min(len(convs), rng.randint(1, 3))):
        q = out[name]
        q["output_bit"] = q["output_bit"] + rng.choice((-2, -1, 1, 1, 2)) if rng.random() < 0.8 else rng.choice((-3, -2, 6))
        q["bias_bit"] = q["output_bit"]
    if net is not None:
        g = Graph(net)
        for name in g.calls:
            if g.kind(name) == "act":
                rd = [r for r in g.readers.get(g.out_of(name)[0], []) if g.kind(r) in ("dense", "depthwise", "grouped")]
                if len(rd) >= 2:
                    out[rd[-1]]["input_bit"] = out[rd[-1]]["input_bit"] - 1
                    break
    return out


# ---------------------------------------------------------------- calibration on the oracle-backed engine
def float_model(index, seed):
    """Model `index` of the family in eval mode, its BatchNorms folded (the flow's first step)."""
    m = RandomMixedNet(index, seed).eval()
    return _cq.merge_bn(m) if m.has_bn else m


def inputs(model, index, seed):
    """(x, x2): the test batch and a flipped, scaled one."""
    x = batches(model, index, seed)[0][0]
    return x, torch.flip(x, dims=[0]) * 0.5


def calibrated(index, seed, builders, per_channel=False, record=None):
    """Calibrate model `index` with the oracle-backed CPU engine (tests/engine_doubles.py), quantise and rewrite its weights, and
    rebuild it as the integer-simulation model once per entry of `builders` -- context managers under which ReconModel runs
    (all_doubles.installed for the host doubles, contextlib.nullcontext for the library).  -> (info, [net, ...]); every net is on the
    host.  With `per_channel` the grouped and depthwise layers take Reconstruction.get_quantity_information_per_channel()'s lists
    (the dense doubles take per-tensor shifts only, so the dense layers keep the per-tensor bits).  `record`, a dict, is filled with
    what golden G22 holds of the flow: graph discovery, merge groups, the tables as written and as rewritten, the layers."""
    import contextlib
    import io
    import os
    from engine_doubles import OracleCollector, OracleQuantizer
    from tools import Quantity, Reconstruction
    from workdir_util import product_workdir

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

        def _weight_row_max(self, tensors):
            from oracle import fq_oracle as orc
            return [np.array([orc.absmax(t[c].numpy()) for c in range(t.shape[0])], dtype=np.float32) for t in tensors]

    model = float_model(index, seed)
    data = batches(model, index, seed)
    nets = []
    with product_workdir(input_shape="1,%d,%d,%d" % (model.cin, model.size, model.size), device="cpu", max_cali_img_num=1) as tmp:
        with contextlib.redirect_stdout(io.StringIO()):
            q = CpuQuantity(model)
            wd = os.path.join(tmp, "test", "workdir")
            if record is not None:
                record.update({"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "layers_num": q.layers_num,
                               "cared_op_layer_names": q.cared_op_layer_names, "merge_groups": q.get_merge_groups(q.net_info)})
            q.activation_quantize(data[1:])
            q.weight_quantize()
            if record is not None:
                record["feat_table"] = open(os.path.join(wd, "feat.table")).read()
                record["weight_table"] = open(os.path.join(wd, "weight.table")).read()
            if per_channel:
                q.weight_quantize_per_channel()
            else:
                q.rewrite_weight()
            info = None
            for n, builder in enumerate(builders):
                rec = Reconstruction(float_model(index, seed))
                info = rec.get_quantity_information()
                if record is not None:
                    record["weight_table_rewritten"] = open(os.path.join(wd, "weight.table")).read()
                    record["recon_layers"] = sorted(info.keys())
                if per_channel:
                    listed = rec.get_quantity_information_per_channel()
                    for name, v in info.items():
                        if v.get("layer_type") == "Conv2d" and v["layer"].groups > 1:
                            info[name] = listed[name]
                with builder():
                    nets.append(rec.ReconModel(info, os.path.join(tmp, "test", "workdir", "recon%d.pth" % n)))
    return info, nets
