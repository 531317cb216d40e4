#!/usr/bin/env python3
"""GPU probe: print every native call the six float-convolution wrappers of _native.py make, argument by argument.

    python scripts/float_conv_call_dump.py > calls.txt

_native.lib() is replaced by a recording proxy that forwards every call to the real library.  Each wrapper (conv1x1_f32,
conv_kxk_f32, dwconv_f32, gconv_f32, conv_stem_f32, conv_wino_f32) is called in each of its forms -- plain, no bias, caller's
out, abs-max, histogram, ReLU copy with and without y, QuanDequan, and the calls that must raise -- on the smallest shape its
kernel accepts, two images each.  One line per native call: the function and every argument, pointers as
<tensor>+<byte offset>, `ws` (the tail-split workspace), `stream` or `null`; for a call that raises, the exception's type and
message.  The output of the tree before a change of the wrappers is the specification of the tree after it:
tests/golden/g17_float_conv_calls.txt, compared by tests/test_gpu_float_conv_calls.py.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-quantity_amd", "quantity"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from common.quantity import _native as nat  # noqa: E402
from native_call_record import Recorder, show_arg  # noqa: E402


def _smallest_wino():
    """The smallest (cin, side, cout) for which the Winograd kernel takes x [2, cin, side, side] -> cout channels."""
    for cin in range(1, 65):
        for cout in range(1, 257):
            for side in range(1, 9):
                if nat.conv_wino_supported(2, cin, side, side, cout):
                    return cin, side, cout
    raise RuntimeError("no small Winograd shape")


def _smallest_sb():
    for cin in range(1, 129):
        for cout in range(1, 65):
            if nat.conv_sb_supported(cin, cout):
                return cin, cout
    raise RuntimeError("no small split-bf16 shape")


def _cases():
    """(label, wrapper, x, the weight operand's name and tensor, positional arguments behind x, output shape, forms or None: all)"""
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(17)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    out = []
    wt = rnd(8, 16).t().contiguous()                                                  # [Cin, Cout]
    out.append(("c1", nat.conv1x1_f32, rnd(2, 16, 5, 5), "wt", wt, lambda b: (wt, b, 1), (2, 8, 5, 5), None))
    out.append(("c1s2", nat.conv1x1_f32, rnd(2, 16, 5, 5), "wt", wt, lambda b: (wt, b, 2), (2, 8, 3, 3), None))
    scin, scout = _smallest_sb()
    wsb = nat.pack_sb_weight(rnd(scout, scin))
    out.append(("c1sb[%d->%d]" % (scin, scout), nat.conv1x1_f32, rnd(2, scin, 5, 5), "wt", wsb, lambda b: (wsb, b, 1), (2, scout, 5, 5),
                ("plain", "max", "hist", "relu+y", "qd5")))
    wk = nat.pack_kxk_weight(rnd(8, 16, 3, 3))
    out.append(("kxk", nat.conv_kxk_f32, rnd(2, 16, 5, 5), "wt", wk, lambda b: (wk, b, (3, 3), 1, 1), (2, 8, 5, 5), None))
    wd = rnd(4, 1, 3, 3)
    out.append(("dw", nat.dwconv_f32, rnd(2, 4, 5, 5), "w", wd, lambda b: (wd, b, (3, 3), 1, 1), (2, 4, 5, 5), None))
    wg = rnd(8, 4, 3, 3)
    out.append(("g", nat.gconv_f32, rnd(2, 8, 5, 5), "w", wg, lambda b: (wg, b, 2, (3, 3), 1, 1), (2, 8, 5, 5), None))
    wp = nat.pack_stem_weight(rnd(8, 3, 7, 7))
    out.append(("stem", nat.conv_stem_f32, rnd(2, 3, 16, 16), "wp", wp, lambda b: (wp, b, 8, (7, 7), 2, 3), (2, 8, 8, 8), None))
    wcin, side, wcout = _smallest_wino()
    u = nat.pack_wino_weight(rnd(wcout, wcin, 3, 3))
    out.append(("wino[%d,%d,%d->%d]" % (wcin, side, side, wcout), nat.conv_wino_f32, rnd(2, wcin, side, side), "u", u,
                lambda b: (u, b, wcout), (2, wcout, side, side), None))
    return out


def dump():
    """The lines of the record (no trailing newlines).  Leaves _native as it found it."""
    assert torch.cuda.is_available(), "float_conv_call_dump needs the GPU"
    real = nat.lib()
    cases = _cases()
    dev = torch.device("cuda")
    ws_ptr, _ = nat.conv_workspace(torch.empty(1, device=dev))                        # allocated before anything is recorded
    lines = []
    rec = Recorder(real)
    nat._lib = rec
    try:
        for label, fn, x, wname, weight, args, shape, forms in cases:
            bias = torch.randn(shape[1], generator=torch.Generator().manual_seed(3)).to(dev)
            mx = torch.zeros(3, device=dev)
            iv = torch.ones(3, device=dev)
            hist = torch.zeros(3, nat.BINS, dtype=torch.int64, device=dev)
            relu = torch.empty(shape, device=dev)
            mine = torch.empty(shape, device=dev)
            bad = torch.empty(shape[:3] + (shape[3] + 1,), device=dev)
            named = (("x", x), (wname, weight), ("bias", bias), ("max", mx), ("iv", iv), ("hist", hist), ("relu", relu), ("out", mine),
                     ("bad", bad))

            def show(a, y):
                if ws_ptr is not None and a == ws_ptr:
                    return "ws"
                return show_arg(a, named + ((("y", y),) if y is not None else ()))

            table = (
                ("plain", x, bias, {}),
                ("nobias", x, None, {}),
                ("out", x, bias, dict(out=mine)),
                ("max", x, bias, dict(max_dev=mx, row=1)),
                ("hist", x, bias, dict(interval_dev=iv, hist_dev=hist, row=1)),
                ("relu+y", x, bias, dict(relu_out=relu)),
                ("relu-only", x, bias, dict(relu_out=relu, out=False)),
                ("qd5", x, bias, dict(qd=5)),
                ("qd5,16", x, bias, dict(qd=(5, 16))),
                ("qd+max", x, bias, dict(qd=5, max_dev=mx, row=1)),
                ("cpu-x", x.cpu(), bias, {}),
                ("fp16-x", x.half(), bias, {}),
                ("bad-out", x, bias, dict(out=bad)),
                ("no-y-no-relu", x, bias, dict(out=False)),
            )
            for form, xin, b, kw in table:
                if forms is not None and form not in forms:
                    continue
                del rec.calls[:]
                y = err = None
                try:
                    y = fn(xin, *args(b), **kw)
                except Exception as e:                                                # the record holds what was raised
                    err = ("%s: %s" % (type(e).__name__, e)).rstrip(": ")
                for name, a in rec.calls:
                    lines.append("%s %s: %s(%s)" % (label, form, name, ", ".join(show(v, y) for v in a)))
                if err is not None:
                    lines.append("%s %s: raises %s" % (label, form, err))
                elif y is not None:
                    lines.append("%s %s: returns %s" % (label, form, "out" if y is mine else "y%s" % (list(y.shape),)))
                else:
                    lines.append("%s %s: returns None" % (label, form))
        torch.cuda.synchronize()
    finally:
        nat._lib = real
    return lines


if __name__ == "__main__":
    print("\n".join(dump()))
