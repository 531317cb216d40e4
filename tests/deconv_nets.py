"""What the transposed-convolution tests share: the kernel's cases, the integer rule of include/fq.h in numpy, the float64
reference with the oracle's tail, and the small calibrated-by-hand networks of the plan tests.

TEST INFRASTRUCTURE: the product never imports this.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import fq_oracle as orc

# (kernel, stride, pad, output_padding) on both axes
KSPO = ((2, 2, 0, 0), (3, 2, 1, 1), (4, 2, 1, 0), (3, 1, 1, 0), (4, 4, 0, 0), (2, 4, 0, 0), (5, 3, 2, 1))
PLANES = ((1, 1), (2, 3), (5, 4), (8, 8))
CK = ((1, 1), (3, 5), (16, 16), (17, 33), (40, 64), (3, 33), (17, 5), (16, 64), (40, 1), (1, 16), (40, 33), (3, 5))
SHIFTS = (1, 7, 16)
BLOCK_PIX, MAX_BLOCKS = 128, 2048


def pad16(c):
    return (int(c) + 15) // 16 * 16


def case(N, H, W, C, K, kernel, stride, pad, outpad, rs=7, relu=0, clip=None):
    return dict(N=N, H=H, W=W, C=C, K=K, kernel=tuple(kernel), stride=tuple(stride), pad=tuple(pad), outpad=tuple(outpad), rs=rs,
                relu=relu, clip=clip)


def kernel_cases():
    """Pairs, not the full product: every (k, s, p, op) meets every plane and, over the list, every (C, K) pair, shift, batch size
    and both ReLU settings."""
    out = []
    n = 0
    for ki, (k, s, p, op) in enumerate(KSPO):
        for pi, (H, W) in enumerate(PLANES):
            if (H - 1) * s - 2 * p + k + op < 1 or (W - 1) * s - 2 * p + k + op < 1:
                continue
            C, K = CK[(ki * 4 + pi) % len(CK)]
            out.append(case((1, 3)[n % 2], H, W, C, K, (k, k), (s, s), (p, p), (op, op), rs=SHIFTS[n % 3], relu=(n // 2) % 2))
            n += 1
    # the rectangle; an `_act` range; an odd chunk count with one channel chunk (3 x 1 taps of one phase)
    out.append(case(3, 5, 4, 16, 64, (2, 3), (2, 1), (0, 0), (0, 0), rs=7))
    out.append(case(1, 5, 4, 17, 33, (3, 2), (1, 2), (1, 0), (0, 1), rs=1, relu=1))
    out.append(case(3, 8, 8, 17, 33, (3, 3), (2, 2), (1, 1), (1, 1), rs=7, clip=(0, 96)))
    out.append(case(1, 2, 3, 40, 5, (4, 4), (2, 2), (1, 1), (0, 0), rs=16, clip=(-7, 5)))
    out.append(case(1, 7, 5, 16, 16, (3, 1), (1, 1), (1, 0), (0, 0), rs=7))
    return out


# more items than the capped grid has workgroups: 66 pixel tiles x 2 channel blocks x 16 phases
BIG_CASE = case(8, 32, 33, 3, 70, (2, 2), (4, 4), (0, 0), (1, 2), rs=1)


def model_launches():
    """The launch shapes of UNet(up="deconv"): base_width 8, depth 2 at 32 x 32, batch 2 (the GPU tests), kernels 2, 3, 4; and
    base_width 32, depth 4 at 224 x 224 (scripts/deconv_cost.py), one image, kernels 2 and 4."""
    out = []
    for k, s, p, op in ((2, 2, 0, 0), (3, 2, 1, 1), (4, 2, 1, 0)):
        out += [case(2, 8, 8, 32, 16, (k, k), (s, s), (p, p), (op, op)), case(2, 16, 16, 16, 8, (k, k), (s, s), (p, p), (op, op))]
    for k, s, p, op in ((2, 2, 0, 0), (4, 2, 1, 0)):
        out += [case(1, 14 << j, 14 << j, 512 >> j, 256 >> j, (k, k), (s, s), (p, p), (op, op)) for j in range(4)]
    return out


def case_id(c):
    return "n%d_%dx%d_c%d_k%d_r%dx%d_s%dx%d_p%dx%d_o%dx%d_rs%d_%s" % (
        c["N"], c["H"], c["W"], c["C"], c["K"], c["kernel"][0], c["kernel"][1], c["stride"][0], c["stride"][1], c["pad"][0],
        c["pad"][1], c["outpad"][0], c["outpad"][1], c["rs"], "act" if c["clip"] else ("relu" if c["relu"] else "lin"))


def out_hw(c):
    return ((c["H"] - 1) * c["stride"][0] - 2 * c["pad"][0] + c["kernel"][0] + c["outpad"][0],
            (c["W"] - 1) * c["stride"][1] - 2 * c["pad"][1] + c["kernel"][1] + c["outpad"][1])


def items(c):
    P, Q = out_hw(c)
    pj, qj = -(-P // c["stride"][0]), -(-Q // c["stride"][1])
    kpad = pad16(c["K"])
    return -(-c["N"] * pj * qj // BLOCK_PIX) * -(-kpad // (64 if kpad > 32 else 32)) * c["stride"][0] * c["stride"][1]


def operands(rng, c):
    """x int8 NHWC with garbage in its padding channels, w int64 [C, K, R, S] over the full int8 range (-128 included), a bias that
    saturates both ways on some channels."""
    cpad = pad16(c["C"])
    x = rng.integers(-128, 128, size=(c["N"], c["H"], c["W"], cpad), dtype=np.int64).astype(np.int8)
    w = rng.integers(-128, 128, size=(c["C"], c["K"]) + c["kernel"], dtype=np.int64)
    x.reshape(-1)[0] = -128
    w.reshape(-1)[0] = -128
    qb = rng.integers(-40, 41, size=c["K"]).astype(np.float32)
    big = np.array([300.0, -300.0, 1e6, -1e6, 3e9, -3e9], dtype=np.float32)
    idx = rng.permutation(c["K"])[:min(c["K"], 6)]
    qb[idx] = big[:idx.size]
    return x, w, qb


def rule_acc(x, w, c):
    """include/fq.h's rule, literally: acc[n][oh][ow][k] as int64, by scattering every tap."""
    C, K = c["C"], c["K"]
    (R, S), (sh, sw), (ph, pw) = c["kernel"], c["stride"], c["pad"]
    P, Q = out_hw(c)
    xi = x[..., :C].astype(np.int64)
    acc = np.zeros((c["N"], P, Q, K), dtype=np.int64)
    for r in range(R):
        for s in range(S):
            contrib = xi @ w[:, :, r, s]                                                   # [N, H, W, K]
            for ih in range(c["H"]):
                oh = ih * sh - ph + r
                if not 0 <= oh < P:
                    continue
                for iw in range(c["W"]):
                    ow = iw * sw - pw + s
                    if 0 <= ow < Q:
                        acc[:, oh, ow] += contrib[:, ih, iw]
    return acc


def f64_acc(x, w, c):
    """The same sums from torch's own transposed convolution in float64 (exact: every partial sum is far below 2^53)."""
    xi = torch.from_numpy(x[..., :c["C"]].astype(np.float64)).permute(0, 3, 1, 2)
    y = F.conv_transpose2d(xi, torch.from_numpy(w.astype(np.float64)), None, c["stride"], c["pad"], c["outpad"])
    return y.permute(0, 2, 3, 1).numpy()


def oracle_tail(acc, qb, c):
    """The oracle's RightShift + BiasAdd + Sp on the accumulators [N, P, Q, K] (below 2^24: exact in fp32), then the ReLU or the
    Sp range of the `_act` entry point (include/fq.h); int8 NHWC with zero padding channels."""
    assert np.abs(acc).max() < 2 ** 24
    a = np.ascontiguousarray(np.moveaxis(acc, -1, 1), dtype=np.float32)                    # [N, K, P, Q]
    y = orc.recon_epilogue(a, qb.astype(np.float32), c["rs"], 0)                           # ob = 0: the integers themselves
    lo, hi = c["clip"] if c["clip"] else ((0, 127) if c["relu"] else (-128, 127))
    y = np.clip(y, lo, hi)
    out = np.zeros(acc.shape[:3] + (pad16(c["K"]),), dtype=np.int8)
    out[..., :c["K"]] = np.moveaxis(y, 1, -1).astype(np.int8)
    return out


def int_tail(acc, qb, c):
    """The tail in integers, as include/fq.h words it: round half away, saturate to [-128, 127], add the bias, Sp range."""
    rs = c["rs"]
    r = np.where(acc >= 0, (acc + (1 << (rs - 1))) >> rs, -((-acc + (1 << (rs - 1))) >> rs))
    r = np.clip(r, -128, 127) + np.clip(qb.astype(np.float64), -1e9, 1e9).astype(np.int64)
    lo, hi = c["clip"] if c["clip"] else ((0, 127) if c["relu"] else (-128, 127))
    out = np.zeros(acc.shape[:3] + (pad16(c["K"]),), dtype=np.int8)
    out[..., :c["K"]] = np.clip(np.clip(r, -128, 127), lo, hi).astype(np.int8)
    return out


def pack_rule(w, c):
    """The packed weights by include/fq.h's words, byte by byte (numpy int8, flat)."""
    C, K = c["C"], c["K"]
    (R, S), (sh, sw), (ph, pw) = c["kernel"], c["stride"], c["pad"]
    cpad, kpad = pad16(C), pad16(K)
    parts = []
    for fh in range(sh):
        for fw in range(sw):
            a, b = (fh + ph) % sh, (fw + pw) % sw
            rows, cols = list(range(a, R, sh)), list(range(b, S, sw))
            blk = np.zeros((kpad, len(rows), len(cols), cpad), dtype=np.int8)
            for th, r in enumerate(rows):
                for tw, s in enumerate(cols):
                    blk[:K, th, tw, :C] = w[:, :, r, s].T.astype(np.int8)
            parts.append(blk.reshape(-1))
    return np.concatenate(parts)


def unpack_rule(pack, c):
    """The [C, K, R, S] int64 weights read back out of a pack (the inverse of pack_rule)."""
    C, K = c["C"], c["K"]
    (R, S), (sh, sw), (ph, pw) = c["kernel"], c["stride"], c["pad"]
    cpad, kpad = pad16(C), pad16(K)
    w = np.zeros((C, K, R, S), dtype=np.int64)
    at = 0
    for fh in range(sh):
        for fw in range(sw):
            a, b = (fh + ph) % sh, (fw + pw) % sw
            rows, cols = list(range(a, R, sh)), list(range(b, S, sw))
            n = kpad * len(rows) * len(cols) * cpad
            blk = pack[at:at + n].reshape(kpad, len(rows), len(cols), cpad)
            at += n
            for th, r in enumerate(rows):
                for tw, s in enumerate(cols):
                    w[:, :, r, s] = blk[:K, th, tw, :C].T
    assert at == pack.size
    return w


def phase_acc(x, pack, c):
    """The kernel's own form in numpy: sub-pixel phase after phase, each a dense stride-1 correlation over ALL Cpad channels of x
    (its padding channels meet the pack's zeros) with that phase's taps; a phase without a tap leaves zeros.  [N, P, Q, K] int64."""
    C, K = c["C"], c["K"]
    (R, S), (sh, sw), (ph, pw) = c["kernel"], c["stride"], c["pad"]
    H, W = c["H"], c["W"]
    P, Q = out_hw(c)
    cpad, kpad = pad16(C), pad16(K)
    xi = x.astype(np.int64)
    acc = np.zeros((c["N"], P, Q, kpad), dtype=np.int64)
    at = 0
    for fh in range(sh):
        for fw in range(sw):
            a, dh, b, dw = (fh + ph) % sh, (fh + ph) // sh, (fw + pw) % sw, (fw + pw) // sw
            Th, Tw = len(range(a, R, sh)), len(range(b, S, sw))
            n = kpad * Th * Tw * cpad
            blk = pack[at:at + n].reshape(kpad, Th, Tw, cpad).astype(np.int64)
            at += n
            for th in range(Th):
                for tw in range(Tw):
                    for j in range(len(range(fh, P, sh))):
                        ih = j + dh - th
                        if not 0 <= ih < H:
                            continue
                        for i in range(len(range(fw, Q, sw))):
                            iw = i + dw - tw
                            if 0 <= iw < W:
                                acc[:, fh + sh * j, fw + sw * i] += xi[:, ih, iw] @ blk[:, th, tw].T
    assert at == pack.size and not acc[..., K:].any()
    return acc[..., :K]


# ---------------------------------------------------------------- small integer-simulation nets, built without calibration
def example(n=4, size=8, seed=1):
    return torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(seed))


def deconv(cin, cout, k, ib, ob, stride=2, padding=0, output_padding=0, seed=0, weight_bit=None, **kw):
    """A NewConvTranspose2d over a seeded nn.ConvTranspose2d whose weights fill the int8 range at the weight bit chosen from their
    abs-max (concat_nets.conv's recipe)."""
    import math
    from common.quantity import NewConvTranspose2d
    gen = torch.Generator().manual_seed(1000 * cin + 10 * cout + k + seed + 77)
    c = nn.ConvTranspose2d(cin, cout, k, stride=stride, padding=padding, output_padding=output_padding, **kw)
    taps = max(1, -(-k // stride)) ** 2
    with torch.no_grad():
        c.weight.copy_(torch.randn(c.weight.shape, generator=gen) * (1.5 / (cin * taps / kw.get("groups", 1)) ** 0.5))
        c.bias.copy_(torch.randn(cout, generator=gen) * 0.2)
    wb = 7 - int(math.ceil(math.log2(float(c.weight.detach().abs().max())))) if weight_bit is None else weight_bit
    return NewConvTranspose2d(c, {"weight_bit": wb, "bias_bit": ob, "input_bit": ib, "output_bit": ob})


TOY_VARIANTS = ("conv_dc_conv", "dc_relu", "dc_relu6", "dc_cat", "dc_cat_rq", "dc_add", "act_dc", "pool_dc", "dc_out")


class ToyNet(nn.Module):
    """stem (3 -> 16, 3x3) + ReLU at bit 4 on the full plane, `down` (16 -> 16, 3x3, stride 2) + ReLU on the half plane, a 1x1
    convolution `a`, the transposed convolution `up` back to the full plane and, by `variant`:
      "conv_dc_conv"  a -> up (2x2, stride 2) -> head (3x3)
      "dc_relu"       a -> up (3x3, stride 2, padding 1, output_padding 1) + ReLU -> head: the ReLU is the up-convolution's
      "dc_relu6"      a -> up (4x4, stride 2, padding 1) + ReLU6 -> head, with relu6=True: the clip is the up-convolution's
      "dc_cat"        Concat(up(a(down)), skip(stem)) -> head, with concat=True: both operands on one grid
      "dc_cat_rq"     ... on two grids, the head at the coarser one, with concat=True, requant=True: the lossy value's reader is
                      a convolution, its operand an integer producer
      "dc_add"        NewAdd(up(a(down)), skip(stem)) -> head
      "act_dc"        a -> LeakyReLU -> up at another bit than a's grid, with activations=True: the table's lossy value is read by
                      the up-convolution, an integer convolution at that bit
      "pool_dc"       a (full plane) + ReLU -> MaxPool2d(2) -> up -> head
      "dc_out"        a -> up is the model output
    `fronts`: the producers that go from emit_f32 to integers only; `kw`: further enable() arguments of both arms."""

    def __init__(self, variant):
        from concat_nets import conv
        from common.quantity import Concat, NewAdd
        super(ToyNet, self).__init__()
        assert variant in TOY_VARIANTS
        self.variant = v = variant
        self.kw, self.fronts = {}, ("a",)
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.down, self.r1 = conv(16, 16, 3, 4, 4, stride=2, padding=1), nn.ReLU()
        self.a = conv(16, 16, 1, 4, 4)
        if v == "conv_dc_conv":
            self.up, self.head = deconv(16, 8, 2, 4, 4), conv(8, 8, 3, 4, 4, padding=1, seed=5)
        elif v == "dc_relu":
            self.up, self.ru = deconv(16, 8, 3, 4, 3, padding=1, output_padding=1), nn.ReLU()
            self.head = conv(8, 8, 1, 3, 4, seed=5)
        elif v == "dc_relu6":
            self.up, self.ru, self.kw = deconv(16, 8, 4, 4, 4, padding=1), nn.ReLU6(), dict(relu6=True)
            self.head = conv(8, 8, 1, 4, 4, seed=5)
        elif v in ("dc_cat", "dc_cat_rq"):
            g = 4 if v == "dc_cat" else 3
            self.up, self.skip, self.cat = deconv(16, 8, 2, 4, g), conv(16, 16, 1, 4, 4, seed=2), Concat()
            self.head = conv(24, 8, 1, g, 4, seed=5)
            self.kw = dict(concat=True) if v == "dc_cat" else dict(concat=True, requant=True)
        elif v == "dc_add":
            self.up, self.skip, self.add = deconv(16, 16, 2, 4, 4), conv(16, 16, 1, 4, 4, seed=2), NewAdd()
            self.head, self.fronts = conv(16, 8, 1, 4, 4, seed=5), ("a", "skip")
        elif v == "act_dc":
            self.act, self.up, self.kw = nn.LeakyReLU(0.1), deconv(16, 8, 2, 3, 4), dict(activations=True)
            self.head = conv(8, 8, 1, 4, 4, seed=5)
        elif v == "pool_dc":
            self.ra, self.pool, self.up = nn.ReLU(), nn.MaxPool2d(2), deconv(16, 8, 2, 4, 4)
            self.head, self.fronts = conv(8, 8, 1, 4, 4, seed=5), ("pool",)
        else:
            self.up = deconv(16, 3, 2, 4, 4)

    def forward(self, x):
        v = self.variant
        s = self.r0(self.stem(x))
        d = self.r1(self.down(s))
        if v == "conv_dc_conv":
            return self.head(self.up(self.a(d)))
        if v in ("dc_relu", "dc_relu6"):
            return self.head(self.ru(self.up(self.a(d))))
        if v in ("dc_cat", "dc_cat_rq"):
            return self.head(self.cat(self.up(self.a(d)), self.skip(s)))
        if v == "dc_add":
            return self.head(self.add(self.up(self.a(d)), self.skip(s)))
        if v == "act_dc":
            return self.head(self.up(self.act(self.a(d))))
        if v == "pool_dc":
            return self.head(self.up(self.pool(self.ra(self.a(s)))))
        return self.up(self.a(d))


DECLINED = {"groups": "groups 2", "dilation": "dilation (2, 2)", "kernel": "a geometry the kernel refuses", "shift": "shift 17 outside [1, 16]",
            "twice": "more than once"}


class DeclinedNet(nn.Module):
    """stem + ReLU at bit 4, a (1x1) on grid 4, `up` and a 1x1 head -- planned as it stands ("ok") -- and by `variant` one thing that
    leaves `up` an fp32 producer (the keys of DECLINED).  "shift": a weight bit of 17 makes the layer's shift 17."""

    def __init__(self, variant):
        from concat_nets import conv
        super(DeclinedNet, self).__init__()
        assert variant == "ok" or variant in DECLINED
        self.variant = v = variant
        self.stem, self.r0 = conv(3, 16, 3, 5, 4, padding=1), nn.ReLU()
        self.a = conv(16, 16, 1, 4, 4)
        if v == "groups":
            self.up = deconv(16, 8, 2, 4, 4, groups=2)
        elif v == "dilation":
            self.up = deconv(16, 8, 2, 4, 4, dilation=2)
        elif v == "kernel":
            self.up = deconv(16, 8, 9, 4, 4, padding=4, output_padding=1)
        elif v == "shift":
            self.up = deconv(16, 8, 2, 4, 4, weight_bit=17)
        elif v == "twice":
            self.up = deconv(16, 16, 3, 4, 4, stride=1, padding=1)
        else:
            self.up = deconv(16, 8, 2, 4, 4)
        self.head = conv(16 if v == "twice" else 8, 8, 1, 4, 4, seed=9)

    def forward(self, x):
        y = self.up(self.a(self.r0(self.stem(x))))
        if self.variant == "twice":
            y = self.up(y)
        return self.head(y)


# ---------------------------------------------------------------- golden G28
G28_SHAPE = (4, 3, 16, 16)
G28_SEED, G28_CALIB_SEED, G28_INPUT_SEED = 28, 2800, 2828


class G28Net(nn.Module):
    """The FLOAT net calibrated for golden G28: conv1 + ReLU (16 px, 8 ch) -> up1 = ConvTranspose2d(8 -> 8, 2, stride 2) (32 px) ->
    ReLU -> conv2 -> up2 = ConvTranspose2d(8 -> 4, 4, stride 2, padding 1) (64 px) -> conv3.  `head_only`: the net ends behind
    conv2, the first up-convolution's consumer (the twin construction)."""

    def __init__(self, head_only=False):
        super(G28Net, self).__init__()
        self.head_only = head_only
        self.conv1, self.relu1 = nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(False)
        self.up1, self.relu2 = nn.ConvTranspose2d(8, 8, 2, stride=2), nn.ReLU(False)
        self.conv2 = nn.Conv2d(8, 8, 3, 1, 1)
        if not head_only:
            self.up2 = nn.ConvTranspose2d(8, 4, 4, stride=2, padding=1)
            self.conv3 = nn.Conv2d(4, 3, 3, 1, 1)

    def forward(self, x):
        x = self.conv2(self.relu2(self.up1(self.relu1(self.conv1(x)))))
        return x if self.head_only else self.conv3(self.up2(x))


class G28Twin(nn.Module):
    """G28Net(head_only=True) with the kernel == stride layer spelled as a 1x1 convolution to 4 K channels + PixelShuffle(2); the
    convolution keeps the name `up1`, so both nets write the same table rows."""

    def __init__(self):
        super(G28Twin, self).__init__()
        self.conv1, self.relu1 = nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(False)
        self.up1, self.shuffle, self.relu2 = nn.Conv2d(8, 32, 1), nn.PixelShuffle(2), nn.ReLU(False)
        self.conv2 = nn.Conv2d(8, 8, 3, 1, 1)

    def forward(self, x):
        return self.conv2(self.relu2(self.shuffle(self.up1(self.relu1(self.conv1(x))))))


def g28_weights(model, seed=G28_SEED):
    """Fixed integer-valued weights, by parameter name and shape (activation_nets.integer_weights, every layer dense)."""
    import activation_nets as an
    return an.integer_weights(model, base_seed=seed, dense=("conv1", "conv2", "conv3", "up1", "up2"))


def g28_net(head_only=False, seed=G28_SEED):
    return g28_weights(G28Net(head_only), seed).eval()


def g28_twin(seed=G28_SEED):
    """The twin of g28_net(head_only=True): W.permute(1, 2, 3, 0).reshape(4 K, C, 1, 1) and b.repeat_interleave(4)."""
    src = g28_net(head_only=True, seed=seed)
    twin = G28Twin()
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    w, b = sd["up1.weight"], sd["up1.bias"]                                # [C, K, 2, 2], [K]
    sd["up1.weight"] = w.permute(1, 2, 3, 0).reshape(4 * w.shape[1], w.shape[0], 1, 1).contiguous()
    sd["up1.bias"] = b.repeat_interleave(4)
    twin.load_state_dict(sd)
    return twin.eval()


def rebuild(float_model, info):
    """depthwise_nets.rebuild with an nn.ConvTranspose2d swapped too: the integer-simulation model from a quantity-information
    dict, without a calibration."""
    import copy
    from common.quantity import NewAdd, NewConv2d, NewConvTranspose2d, NewLinear
    model = copy.deepcopy(float_model)
    for name, mod in list(model.named_modules()):
        kind = type(mod).__name__
        if kind in ("Conv2d", "Linear", "ConvTranspose2d"):
            q = {k: v for k, v in info[name].items() if k not in ("layer", "layer_type")}
            new = {"Conv2d": NewConv2d, "Linear": NewLinear, "ConvTranspose2d": NewConvTranspose2d}[kind](mod, q)
        elif kind == "Eltwise":
            new = NewAdd()
        else:
            continue
        parent = model
        for p in name.split(".")[:-1]:
            parent = getattr(parent, p)
        parent.add_module(name.split(".")[-1], new)
    return model.eval()


# ---------------------------------------------------------------- the random family
class RandomDeconvNet(nn.Module):
    """A random integer-simulation net drawn from `seed`: plane 3 to 6, batch 4, widths 3 to 40, bits 2 .. 5, a stem and two or three
    stages.  A stage reads an int8 activation and draws one up-convolution -- geometry from deconv_nets.KSPO and a rectangle, now and
    then with groups 2, dilation 2 or at a weight bit that puts the shift outside [1, 16] (declined) -- with a ReLU, a ReLU6 or
    nothing behind it, then a convolution (now and then at another bit, so that it reads fp32) with stride 2 or a max-pool that
    brings the plane back.  `ups`: [(module name, expected to be planned)]."""

    def __init__(self, seed):
        from concat_nets import conv
        super(RandomDeconvNet, self).__init__()
        import random
        rng = random.Random(3500 + seed)
        self.plane = rng.choice((3, 4, 5, 6))
        widths = (3, 8, 16, 17, 40)
        cin, ib = rng.choice(widths), rng.randint(3, 5)
        self.stem, self.r0 = conv(3, cin, 3, 5, ib, padding=1, seed=seed), nn.ReLU()
        mods, self.stages, self.ups = {}, [], []
        for j in range(rng.choice((2, 3))):
            k, s, p, op = rng.choice(KSPO[:5] + ((2, 2, 0, 0), (4, 2, 1, 0)))
            bad = rng.choice((None,) * 8 + ("groups", "dilation", "shift"))
            cout, g = rng.choice(widths), rng.randint(2, 5)
            kw = {}
            if bad == "groups":
                cin2 = cin if cin % 2 == 0 else None
                if cin2 is None or cout % 2:
                    bad = None
                else:
                    kw["groups"] = 2
            if bad == "dilation":
                kw["dilation"] = 2
            mods["up%d" % j] = deconv(cin, cout, k, ib, g, stride=s, padding=p, output_padding=op, seed=seed + 10 * j,
                                         weight_bit=17 if bad == "shift" else None, **kw)
            act = rng.choice(("none", "relu", "relu", "relu6"))
            mods["ru%d" % j] = {"none": nn.Identity(), "relu": nn.ReLU(), "relu6": nn.ReLU6()}[act]
            self.ups.append(("mods.up%d" % j, bad is None))
            rb = g if rng.random() < 0.85 else (g + 1 if g < 5 else g - 1)
            nxt, ob = rng.choice(widths), rng.randint(2, 5)
            mods["mix%d" % j], mods["rm%d" % j] = conv(cout, nxt, 3, rb, ob, stride=min(s, 2), padding=1, seed=seed + 10 * j + 4), nn.ReLU()
            mods["pool%d" % j] = nn.MaxPool2d(2) if s == 4 else nn.Identity()
            self.stages.append(j)
            cin, ib = nxt, ob
        self.mods = nn.ModuleDict(mods)
        self.head = conv(cin, 4, 1, ib, 4, seed=seed + 90)

    def example(self, seed=1):
        return torch.randn(4, 3, self.plane, self.plane, generator=torch.Generator().manual_seed(seed))

    def forward(self, x):
        m = self.mods
        x = self.r0(self.stem(x))
        for j in self.stages:
            x = m["ru%d" % j](m["up%d" % j](x))
            x = m["pool%d" % j](m["rm%d" % j](m["mix%d" % j](x)))
        return self.head(x)


SEEDS = list(range(20))


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


def unet_model(**kw):
    """model/unet/UNet_fabu.py's UNet (the product's `common` package must be the imported one)."""
    return _model_file("_fq_unet_fabu_deconv", ("unet", "UNet_fabu.py")).UNet(**kw)
