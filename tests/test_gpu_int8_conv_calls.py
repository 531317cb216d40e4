"""What the integer-convolution wrappers of _native.py hand to the native library, argument by argument: conv2d_i8,
conv2d_i8_resident, conv2d_i8_add_resident, conv2d_i8_stem, dwconv2d_i8_resident, gconv2d_i8_resident, block_tail_i8,
block_tail_proj_i8 and add_resident in every form -- the shift an int, a ShiftVec, for the block tails one ShiftVec among ints;
relu off, on, a clip; every combination of wanted outputs -- and what they raise for a CPU or wrongly typed x, a ShiftVec of the
wrong length or alignment, a clip that excludes 0, no output wanted, a residual of the wrong shape or dtype and a window that
does not fit.  The record (scripts/int8_conv_call_dump.py) was taken from the tree in which every wrapper still carried one
copy of its native call per entry point; the shared call path (_native._conv_i8) has to reproduce it line for line.
    pytest -m gpu"""
import importlib.util
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAMILIES = ("fq_conv2d_i8", "fq_conv2d_i8_resident", "fq_conv2d_i8_stem", "fq_dwconv2d_i8_resident", "fq_gconv2d_i8_resident",
            "fq_conv2d_i8_add_resident")
WITH_ACT = ("fq_conv2d_i8_resident", "fq_conv2d_i8_stem", "fq_dwconv2d_i8_resident", "fq_gconv2d_i8_resident")
ENTRY_POINTS = ([f + p for f in FAMILIES for p in ("", "_pcs")] + [f + p + "_act" for f in WITH_ACT for p in ("", "_pcs")] +
                ["fq_block_tail_i8", "fq_block_tail_i8_pcs", "fq_block_tail_proj_i8", "fq_block_tail_proj_i8_pcs"])


def test_the_wrappers_make_the_recorded_native_calls():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    spec = importlib.util.spec_from_file_location("int8_conv_call_dump", os.path.join(ROOT, "scripts", "int8_conv_call_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from common.quantity import _native
    real = _native.lib()
    got = mod.dump()
    assert _native.lib() is real                                  # the recording proxy is gone again
    with open(os.path.join(ROOT, "tests", "golden", "g19_int8_conv_calls.txt")) as fh:
        want = fh.read().splitlines()
    assert len(got) == len(want), (len(got), len(want))
    for a, b in zip(got, want):
        assert a == b
    assert len(ENTRY_POINTS) == 12 + 8 + 4                        # six families x {plain, _pcs}, the eight _act, the four block tails
    called = set(m.group(1) for m in (re.search(r": (fq_\w+)\(", line) for line in got) if m)
    assert not [e for e in ENTRY_POINTS if e not in called]       # a form list that quietly shrank
