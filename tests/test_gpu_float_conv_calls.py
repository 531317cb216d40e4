"""What the six float-convolution wrappers of _native.py hand to the native library, argument by argument: conv1x1_f32 (fp32 and
split-bf16 pack), conv_kxk_f32, dwconv_f32, gconv_f32, conv_stem_f32 and conv_wino_f32 in every form -- plain, no bias, caller's
out, abs-max and histogram of row 1 of 3, ReLU copy with and without y, QuanDequan at 8 and 16 bits -- and what they raise for a
statistic next to QuanDequan, a CPU or fp16 x, an out of the wrong shape and out=False without a ReLU copy.  The record
(scripts/float_conv_call_dump.py) was taken from the tree in which every wrapper still carried its own copy of the epilogue
plumbing; the shared call path (_native._conv_f32) has to reproduce it line for line.
    pytest -m gpu"""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_wrappers_make_the_recorded_native_calls():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    spec = importlib.util.spec_from_file_location("float_conv_call_dump", os.path.join(ROOT, "scripts", "float_conv_call_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from common.quantity import _native
    real = _native.lib()
    got = mod.dump()
    assert _native.lib() is real                                  # the recording proxy is gone again
    with open(os.path.join(ROOT, "tests", "golden", "g17_float_conv_calls.txt")) as fh:
        want = fh.read().splitlines()
    assert len(got) == len(want), (len(got), len(want))
    for a, b in zip(got, want):
        assert a == b
