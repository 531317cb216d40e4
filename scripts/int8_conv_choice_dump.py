#!/usr/bin/env python3
"""GPU probe: which kernel the dense int8 convolution dispatch launches for every layer of tests/conv_select_cases.py, under every
switch setting of that list.

    python scripts/int8_conv_choice_dump.py > choices.txt
    python scripts/ab_lib.py OTHER/libfq_hip.so scripts/int8_conv_choice_dump.py > choices_other.txt
    python scripts/int8_conv_choice_dump.py --setting "halo8=2"          one setting, in this process (for a profiler)

The sibling of int8_conv_call_dump.py.  The switches are read once per process, so every setting runs in a child process of its
own with the FQ_* variables in its environment (the parent never touches the GPU).  A case is ONE launch through the raw entry
point its outputs ask for -- fq_conv2d_i8 (y), fq_conv2d_i8_resident (q, yq), fq_conv2d_i8_add_resident (add), their _pcs forms --
on zero-filled operands, followed by fq_conv2d_i8_last_variant().  One line per case: `<setting> | <case>: <kernel>/<TK>`.  The
output of the tree before csrc/fq_conv_i8_select.h existed is tests/golden/g21_int8_conv_choice.txt: the selector must name the
same kernel for every row on the host (tests/test_conv_i8_select_cpu.py), and this script must print the same file again.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-quantity_amd", "quantity"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv_select_cases as cs  # noqa: E402

RS, OB, IB, G = 9, 5, 4, 5                    # shift, output grid, narrow grid, the residual's grid (as int8_conv_call_dump.py)


def _launch(nat, torch, text):
    geom, outs = text.split("/")[0], text.split("/")[1:]
    N, H, W, C, K, R, S, sh, sw, ph, pw, dh, dw = (int(v) for v in geom.split(","))
    pcs = outs[1:] == ["pcs"]
    P = (H + 2 * ph - dh * (R - 1) - 1) // sh + 1
    Q = (W + 2 * pw - dw * (S - 1) - 1) // sw + 1
    kpad = (K + 15) // 16 * 16
    dev = torch.device("cuda")
    x = torch.zeros(N, H, W, C, dtype=torch.int8, device=dev)
    w = torch.zeros(K, R, S, C, dtype=torch.int8, device=dev)
    qb = torch.zeros(K, dtype=torch.float32, device=dev)
    y = torch.empty(N, K, P, Q, dtype=torch.float32, device=dev) if outs[0] in ("y", "yq") else None
    q = torch.empty(N, P, Q, kpad, dtype=torch.int8, device=dev) if outs[0] in ("q", "yq", "add") else None
    res = torch.zeros(N, P, Q, kpad, dtype=torch.int8, device=dev) if outs[0] == "add" else None
    rsk = torch.full((K,), RS, dtype=torch.int32, device=dev) if pcs else None
    ptr = lambda t: None if t is None else t.data_ptr()
    geo = (N, H, W, C, K, R, S, sh, sw, ph, pw, dh, dw)
    shift = (ptr(rsk), RS, RS) if pcs else ()
    L, st = nat.lib(), nat._stream(x)
    if outs[0] == "add":
        fn = L.fq_conv2d_i8_add_resident_pcs if pcs else L.fq_conv2d_i8_add_resident
        rc = fn(ptr(x), ptr(w), ptr(qb), *shift, ptr(res), 1, G, None, G, ptr(q), IB, 1, kpad, *geo, *(() if pcs else (RS,)), OB, st)
    elif outs[0] == "y":
        fn = L.fq_conv2d_i8_pcs if pcs else L.fq_conv2d_i8
        rc = fn(ptr(x), ptr(w), ptr(qb), *shift, ptr(y), *geo, *(() if pcs else (RS,)), OB, 8, st)
    else:
        fn = L.fq_conv2d_i8_resident_pcs if pcs else L.fq_conv2d_i8_resident
        rc = fn(ptr(x), ptr(w), ptr(qb), *shift, ptr(y), ptr(q), kpad, 1, *geo, *(() if pcs else (RS,)), OB, st)
    v = int(L.fq_conv2d_i8_last_variant())
    torch.cuda.synchronize()
    if rc != 0:
        return "rc %d" % rc
    return nat.CONV_VARIANTS.get(v & 0xff, "?") + "/%d" % (v >> 8)


def run_setting(name, lib_path=None):
    """The lines of one setting, launched in THIS process: its switches go into the environment before the first launch."""
    _, switches, cases = next(s for s in cs.SETTINGS if s[0] == name)
    for s in switches:
        os.environ[s.split("=", 1)[0]] = s.split("=", 1)[1]
    import torch
    from common.quantity import _native as nat
    if lib_path:
        nat.LIB_PATH = lib_path
    assert torch.cuda.is_available(), "int8_conv_choice_dump needs the GPU"
    return ["%s | %s: %s" % (name, c, _launch(nat, torch, c)) for c in cases]


def dump():
    """Every setting in a child process of its own, one after the other, against the library this process would load."""
    from common.quantity import _native as nat
    lines = []
    for name, _, _ in cs.SETTINGS:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--setting", name, "--lib", nat.LIB_PATH], capture_output=True,
                             text=True, env={k: v for k, v in os.environ.items() if not k.startswith("FQ_")})
        if out.returncode != 0:
            raise SystemExit("setting %r failed (exit %d):\n%s%s" % (name, out.returncode, out.stdout, out.stderr))
        lines += out.stdout.splitlines()
    return lines


if __name__ == "__main__":
    if "--setting" in sys.argv:
        lib = sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else None
        print("\n".join(run_setting(sys.argv[sys.argv.index("--setting") + 1], lib)))
    else:
        print("\n".join(dump()))
