#!/usr/bin/env python3
"""GPU probe: print every native call the integer-convolution wrappers of _native.py make, argument by argument.

    python scripts/int8_conv_call_dump.py > calls.txt

The sibling of float_conv_call_dump.py.  _native.lib() is replaced by a recording proxy that forwards every call to the real
library, and conv_variant_log is switched on so that the fq_conv2d_i8_last_variant calls are part of the record.  conv2d_i8,
conv2d_i8_resident, conv2d_i8_add_resident, conv2d_i8_stem, dwconv2d_i8_resident, gconv2d_i8_resident, block_tail_i8,
block_tail_proj_i8 and add_resident are called in each of their forms -- the shift an int, a ShiftVec, for the block tails also
one ShiftVec among ints; relu off, on, a clip; every combination of wanted outputs; relu1 -- and with the operands that must
raise, on the smallest shape the kernel accepts, two images each.  One line per native call: the function and every argument,
pointers as <operand>+<byte offset>, a returned tensor as ret / ret[i], a cached constant shift vector as const(value,K),
`stream` or `null`; then what was returned (dtype and shape) or raised, and the kernels conv_variant_log counted.  The output of
the tree before a change of the wrappers is the specification of the tree after it: tests/golden/g19_int8_conv_calls.txt,
compared by tests/test_gpu_int8_conv_calls.py.
"""
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-quantity_amd", "quantity"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from common.quantity import _native as nat  # noqa: E402
from native_call_record import Recorder, show_arg  # noqa: E402

RS, OB, IB, G = 9, 5, 4, 5                    # the per-tensor shift, the output grid, the narrow grid, the residual's / wide grid
ACTS = (("relu0", False, None), ("relu1", True, None), ("clip", False, (0, 96)))
WANTS = ((True, False), (False, True), (True, True))


def _cases():
    """[(label, form, wrapper, positional arguments, keyword arguments, ((operand name, tensor), ...))]"""
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(19)

    def i8(*shape):
        return torch.randint(-8, 9, shape, generator=g).to(torch.int8).to(dev)

    def i16(*shape):
        return torch.randint(-300, 301, shape, generator=g).to(torch.int16).to(dev)

    def wf(*shape):                                                                   # integer-valued fp32 weights
        return torch.randint(-8, 9, shape, generator=g).float().to(dev)

    def qb(n):                                                                        # integer-valued fp32 bias
        return torch.randint(-64, 65, (n,), generator=g).float().to(dev)

    def vec(n):                                                                       # a ShiftVec with lo < hi
        return nat.ShiftVec((8 + torch.arange(n, dtype=torch.int32) % 3).to(dev), 8, 10)

    def bad_vecs(n):
        """(form, ShiftVec): one entry too many, and the right length 4 bytes off 16-byte alignment"""
        off = torch.full((n + 1,), RS, dtype=torch.int32, device=dev)
        return (("vec-long", nat.ShiftVec(off, RS, RS)), ("vec-unaligned", nat.ShiftVec(off[1:], RS, RS)))

    out = []

    def add(label, form, fn, args, named, **kw):
        out.append((label, form, fn, tuple(args), kw, tuple(named)))

    def shifts(n):
        return (("int", RS), ("vec", vec(n)))

    def named_rs(rs, name="rs"):
        return ((name, rs.t),) if isinstance(rs, nat.ShiftVec) else ()

    # ---- conv2d_i8, conv2d_i8_resident, conv2d_i8_add_resident: x [2, 5, 5, 16]; 3x3 pad 1 and 1x1 stride 2; Linear x [2, 16]
    x = i8(2, 5, 5, 16)
    xl = i8(2, 16)
    w3, w1 = nat.pack_weight_krsc(wf(8, 16, 3, 3)), nat.pack_weight_krsc(wf(8, 16, 1, 1))
    b = qb(8)
    dense = (("c3", x, w3, (1, 1), (1, 1)), ("c1s2", x, w1, (2, 2), (0, 0)))
    for label, xin, w, st, pd in dense + (("lin", xl, w1, (1, 1), (0, 0)),):
        for sf, rs in shifts(8):
            add("conv2d_i8 " + label, sf, nat.conv2d_i8, (xin, w, b, st, pd, (1, 1), rs, OB), (("x", xin), ("w", w), ("qbias", b)) + named_rs(rs))
    for form, xin, rs in (("cpu-x", x.cpu(), RS), ("fp32-x", x.float(), RS)) + tuple((f, x, v) for f, v in bad_vecs(8)):
        add("conv2d_i8 c3", form, nat.conv2d_i8, (xin, w3, b, (1, 1), (1, 1), (1, 1), rs, OB), (("x", xin), ("w", w3), ("qbias", b)) + named_rs(rs))

    for label, xin, w, st, pd in dense:
        for (sf, rs), (af, relu, clip), (wa, wb) in itertools.product(shifts(8), ACTS, WANTS):
            add("conv2d_i8_resident " + label, "%s %s f32=%d i8=%d" % (sf, af, wa, wb), nat.conv2d_i8_resident,
                (xin, w, b, st, pd, (1, 1), rs, OB, wa, wb, relu), (("x", xin), ("w", w), ("qbias", b)) + named_rs(rs), clip=clip)
    for form, xin, rs, wa, clip in ((("cpu-x", x.cpu(), RS, True, None), ("fp32-x", x.float(), RS, True, None)) +
                                    tuple((f, x, v, True, None) for f, v in bad_vecs(8)) +
                                    (("clip(1,96)", x, RS, True, (1, 96)), ("vec clip(1,96)", x, vec(8), True, (1, 96)),
                                     ("no-output", x, RS, False, None))):
        add("conv2d_i8_resident c3", form, nat.conv2d_i8_resident, (xin, w3, b, (1, 1), (1, 1), (1, 1), rs, OB, wa, False, True),
            (("x", xin), ("w", w3), ("qbias", b)) + named_rs(rs), clip=clip)

    res8, res16 = i8(2, 5, 5, 16), i16(2, 5, 5, 16)

    def conv_add(form, xin, rs, res, ww, wn, relu):
        add("conv2d_i8_add_resident c3", form, nat.conv2d_i8_add_resident,
            (xin, w3, b, (1, 1), (1, 1), (1, 1), rs, OB, res, G, ww, G, wn, IB, relu),
            (("x", xin), ("w", w3), ("qbias", b), ("res", res)) + named_rs(rs))

    for (rf, res), (sf, rs), relu, (ww, wn) in itertools.product((("res8", res8), ("res16", res16)), shifts(8), (False, True), WANTS):
        conv_add("%s %s relu%d wide=%d narrow=%d" % (rf, sf, relu, ww, wn), x, rs, res, ww, wn, relu)
    conv_add("cpu-x", x.cpu(), RS, res8, True, True, True)
    conv_add("fp32-x", x.float(), RS, res8, True, True, True)
    for f, v in bad_vecs(8):
        conv_add(f, x, v, res8, True, True, True)
    conv_add("no-output", x, RS, res8, False, False, True)
    conv_add("res-shape", x, RS, i8(2, 5, 4, 16), True, True, True)
    conv_add("res-fp32", x, RS, res8.float(), True, True, True)

    # ---- conv2d_i8_stem: fp32 [2, 3, 16, 16], 7x7 stride 2 pad 3, K = 8
    xs = torch.randint(-64, 65, (2, 3, 16, 16), generator=g).float().div(32).to(dev)
    ws = nat.pack_weight_stem(wf(8, 3, 7, 7))

    def stem(form, xin, rs, relu, clip):
        add("conv2d_i8_stem", form, nat.conv2d_i8_stem, (xin, ws, b, 8, 7, (2, 2), (3, 3), 5, rs, OB, relu),
            (("x", xin), ("w", ws), ("qbias", b)) + named_rs(rs), clip=clip)

    for (sf, rs), (af, relu, clip) in itertools.product(shifts(8), ACTS):
        stem("%s %s" % (sf, af), xs, rs, relu, clip)
    stem("cpu-x", xs.cpu(), RS, True, None)
    stem("fp16-x", xs.half(), RS, True, None)
    for f, v in bad_vecs(8):
        stem(f, xs, v, True, None)
    stem("clip(1,96)", xs, RS, True, (1, 96))
    stem("vec clip(1,96)", xs, vec(8), True, (1, 96))

    # ---- dwconv2d_i8_resident: C = 4 (Cpad 16), 5 x 5 plane; 3x3 stride 1 pad 1 and 5x5 stride 2 pad 2
    xd = i8(2, 5, 5, 16)
    xd[..., 4:] = 0
    bd = qb(4)
    wd3, wd5 = nat.pack_weight_dw(wf(4, 1, 3, 3)), nat.pack_weight_dw(wf(4, 1, 5, 5))

    def dw(label, form, xin, w, st, pd, rs, relu, clip):
        add("dwconv2d_i8_resident " + label, form, nat.dwconv2d_i8_resident, (xin, w, bd, st, pd, rs, OB, relu),
            (("x", xin), ("w", w), ("qbias", bd)) + named_rs(rs), clip=clip)

    for (label, w, st, pd), (sf, rs), (af, relu, clip) in itertools.product(
            (("3x3", wd3, (1, 1), (1, 1)), ("5x5s2", wd5, (2, 2), (2, 2))), shifts(4), ACTS):
        dw(label, "%s %s" % (sf, af), xd, w, st, pd, rs, relu, clip)
    dw("3x3", "cpu-x", xd.cpu(), wd3, (1, 1), (1, 1), RS, True, None)
    dw("3x3", "fp32-x", xd.float(), wd3, (1, 1), (1, 1), RS, True, None)
    for f, v in bad_vecs(4):
        dw("3x3", f, xd, wd3, (1, 1), (1, 1), v, True, None)
    dw("3x3", "clip(1,96)", xd, wd3, (1, 1), (1, 1), RS, True, (1, 96))
    dw("3x3", "vec clip(1,96)", xd, wd3, (1, 1), (1, 1), vec(4), True, (1, 96))
    x1 = i8(2, 1, 1, 16)
    dw("3x3", "no-fit", x1, wd3, (1, 1), (0, 0), RS, True, None)
    dw("3x3", "vec no-fit", x1, wd3, (1, 1), (0, 0), vec(4), True, None)

    # ---- gconv2d_i8_resident: groups 2, 4 -> 4 channels per group (C = K = 8), 5 x 5 plane; 3x3 pad 1 and 1x1
    xg = i8(2, 5, 5, 16)
    xg[..., 8:] = 0
    wg3, wg1 = nat.pack_weight_grouped(wf(8, 4, 3, 3), 2), nat.pack_weight_grouped(wf(8, 4, 1, 1), 2)

    def gc(label, form, xin, w, pd, rs, relu, clip):
        add("gconv2d_i8_resident " + label, form, nat.gconv2d_i8_resident, (xin, w, b, 8, 2, (1, 1), pd, rs, OB, relu),
            (("x", xin), ("w", w), ("qbias", b)) + named_rs(rs), clip=clip)

    for (label, w, pd), (sf, rs), (af, relu, clip) in itertools.product((("3x3", wg3, (1, 1)), ("1x1", wg1, (0, 0))), shifts(8), ACTS):
        gc(label, "%s %s" % (sf, af), xg, w, pd, rs, relu, clip)
    gc("3x3", "cpu-x", xg.cpu(), wg3, (1, 1), RS, True, None)
    gc("3x3", "fp32-x", xg.float(), wg3, (1, 1), RS, True, None)
    for f, v in bad_vecs(8):
        gc("3x3", f, xg, wg3, (1, 1), v, True, None)
    gc("3x3", "clip(1,96)", xg, wg3, (1, 1), RS, True, (1, 96))
    gc("3x3", "vec clip(1,96)", xg, wg3, (1, 1), vec(8), True, (1, 96))
    gc("3x3", "no-fit", x1, wg3, (0, 0), RS, True, None)
    gc("3x3", "vec no-fit", x1, wg3, (0, 0), vec(8), True, None)

    # ---- block_tail_i8 / block_tail_proj_i8: x [2, 3, 3, 64], K3 = 128, C2 in {0, 64}
    xt = i8(2, 3, 3, 64)
    wt3, bt3 = nat.pack_weight_krsc(wf(128, 64, 1, 1)), qb(128)
    wt1, bt1 = nat.pack_weight_krsc(wf(64, 128, 1, 1)), qb(64)
    rt8, rt16 = i8(2, 3, 3, 128), i16(2, 3, 3, 128)
    v3, v1, vp = vec(128), vec(64), vec(128)
    # which shifts are vectors: none, all, or one among ints (the others then come from _shift_of)
    tail_shifts = (("int", RS, RS, RS), ("vec", v3, v1, vp), ("mix3", v3, RS, RS), ("mix1", RS, v1, RS), ("mixp", RS, RS, vp))

    def tail(form, xin, rs3, res, ww, wn, relu, c2, rs1, relu1):
        kw = dict(w1q=wt1, qbias1=bt1, rs1=rs1, relu1=relu1) if c2 else {}
        add("block_tail_i8 C2=%d" % c2, form, nat.block_tail_i8, (xin, wt3, bt3, rs3, OB, res, G, ww, G, wn, IB, relu),
            (("x", xin), ("w3", wt3), ("qbias3", bt3), ("res", res), ("w1", wt1), ("qbias1", bt1)) + named_rs(rs3, "rs3") +
            named_rs(rs1, "rs1"), **kw)

    for c2 in (0, 64):
        for (rf, res), (sf, rs3, rs1, _), relu, (ww, wn), relu1 in itertools.product(
                (("res8", rt8), ("res16", rt16)), tail_shifts[:4], (False, True), WANTS + ((False, False),), (False, True)):
            if not c2 and (relu1 or sf in ("mix3", "mix1") or not (ww or wn)):          # (without conv1 there is one shift only)
                continue
            tail("%s %s relu%d wide=%d narrow=%d relu1=%d" % (rf, sf, relu, ww, wn, relu1), xt, rs3, res, ww, wn, relu, c2, rs1, relu1)
    tail("cpu-x", xt.cpu(), RS, rt8, True, True, True, 64, RS, True)
    tail("fp32-x", xt.float(), RS, rt8, True, True, True, 64, RS, True)
    for f, v in bad_vecs(128):
        tail("rs3 " + f, xt, v, rt8, True, True, True, 64, RS, True)
    for f, v in bad_vecs(64):
        tail("rs1 " + f, xt, RS, rt8, True, True, True, 64, v, True)
    tail("no-output", xt, RS, rt8, False, False, True, 0, RS, False)
    tail("res-shape", xt, RS, i8(2, 3, 2, 128), True, True, True, 64, RS, True)
    tail("res-fp32", xt, RS, rt8.float(), True, True, True, 64, RS, True)

    wtp, btp = nat.pack_weight_krsc(wf(128, 64, 1, 1)), qb(128)
    xps = {1: i8(2, 3, 3, 64), 2: i8(2, 5, 5, 64)}

    def proj(form, xin, rs3, rsp, sp, ww, wn, relu, c2, rs1, relu1, xp=None):
        xp = xps[sp] if xp is None else xp
        kw = dict(w1q=wt1, qbias1=bt1, rs1=rs1, relu1=relu1) if c2 else {}
        add("block_tail_proj_i8 C2=%d" % c2, form, nat.block_tail_proj_i8,
            (xin, wt3, bt3, rs3, OB, xp, wtp, btp, rsp, G, sp, ww, G, wn, IB, relu),
            (("x", xin), ("w3", wt3), ("qbias3", bt3), ("xp", xp), ("wp", wtp), ("qbiasp", btp), ("w1", wt1), ("qbias1", bt1)) +
            named_rs(rs3, "rs3") + named_rs(rsp, "rsp") + named_rs(rs1, "rs1"), **kw)

    for c2 in (0, 64):
        for sp, (sf, rs3, rs1, rsp), relu, (ww, wn), relu1 in itertools.product(
                (1, 2), tail_shifts, (False, True), WANTS + ((False, False),), (False, True)):
            if not c2 and (relu1 or sf == "mix1" or not (ww or wn)):
                continue
            proj("s%d %s relu%d wide=%d narrow=%d relu1=%d" % (sp, sf, relu, ww, wn, relu1), xt, rs3, rsp, sp, ww, wn, relu, c2, rs1, relu1)
    proj("cpu-x", xt.cpu(), RS, RS, 1, True, True, True, 64, RS, True)
    proj("fp32-x", xt.float(), RS, RS, 1, True, True, True, 64, RS, True)
    proj("fp32-xp", xt, RS, RS, 1, True, True, True, 64, RS, True, xp=xps[1].float())
    for f, v in bad_vecs(128):
        proj("rs3 " + f, xt, v, RS, 1, True, True, True, 64, RS, True)
        proj("rsp " + f, xt, RS, v, 1, True, True, True, 64, RS, True)
    for f, v in bad_vecs(64):
        proj("rs1 " + f, xt, RS, RS, 1, True, True, True, 64, v, True)
    proj("no-output", xt, RS, RS, 1, False, False, True, 0, RS, False)

    # ---- add_resident: int8 + int16 of [2, 3, 3, 16]
    a8, a16 = i8(2, 3, 3, 16), i16(2, 3, 3, 16)

    def addr(form, p, q, ww, wn, relu):
        add("add_resident", form, nat.add_resident, (p, G, q, G, ww, G, wn, IB, relu), (("x", p), ("y", q)))

    for relu, (ww, wn) in itertools.product((False, True), WANTS):
        addr("relu%d wide=%d narrow=%d" % (relu, ww, wn), a8, a16, ww, wn, relu)
    addr("cpu-x", a8.cpu(), a16, True, True, True)
    addr("fp32-x", a8.float(), a16, True, True, True)
    addr("no-output", a8, a16, False, False, True)
    addr("y-shape", a8, i16(2, 3, 2, 16), True, True, True)
    return out


def _describe(y):
    if isinstance(y, tuple):
        return "(%s)" % ", ".join(_describe(v) for v in y)
    if y is None:
        return "None"
    return "%s%s" % (str(y.dtype).replace("torch.", ""), list(y.shape))


def dump():
    """The lines of the record (no trailing newlines).  Leaves _native as it found it."""
    assert torch.cuda.is_available(), "int8_conv_call_dump needs the GPU"
    real = nat.lib()
    cases = _cases()
    lines = []
    rec = Recorder(real)
    log_before = nat.conv_variant_log
    nat._lib = rec
    try:
        for label, form, fn, args, kw, named in cases:
            del rec.calls[:]
            nat.conv_variant_log = {}
            y = err = None
            try:
                y = fn(*args, **kw)
            except Exception as e:                                                    # the record holds what was raised
                err = ("%s: %s" % (type(e).__name__, e)).rstrip(": ")
            where = named
            if isinstance(y, tuple):
                where += tuple(("ret[%d]" % i, t) for i, t in enumerate(y) if t is not None)
            elif y is not None:
                where += (("ret", y),)
            where += tuple(("const(%d,%d)" % (v, k), t) for (v, k, _), t in sorted(nat._CONST_SHIFTS.items()))
            for name, a in rec.calls:
                lines.append("%s | %s: %s(%s)" % (label, form, name, ", ".join(show_arg(v, where) for v in a)))
            if err is not None:
                lines.append("%s | %s: raises %s" % (label, form, err))
            else:
                lines.append("%s | %s: returns %s, kernels %s" % (label, form, _describe(y), sorted(nat.conv_variant_log.items())))
        torch.cuda.synchronize()
    finally:
        nat._lib = real
        nat.conv_variant_log = log_before
    return lines


if __name__ == "__main__":
    print("\n".join(dump()))
