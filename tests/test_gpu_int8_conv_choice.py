"""Golden G21 on the GPU: one launch per layer of tests/conv_select_cases.py's default setting through the raw entry points, and
fq_conv2d_i8_last_variant() after each -- the kernel the dispatcher launched is the one the record of the tree before
csrc/fq_conv_i8_select.h names (scripts/int8_conv_choice_dump.py; the other settings need a process each, the switches being read
once: `python scripts/int8_conv_choice_dump.py | diff - tests/golden/g21_int8_conv_choice.txt`).  The same rows are held on the host by
tests/test_conv_i8_select_cpu.py.
    pytest -m gpu"""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_default_dispatch_launches_the_recorded_kernels():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    spec = importlib.util.spec_from_file_location("int8_conv_choice_dump", os.path.join(ROOT, "scripts", "int8_conv_choice_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    knobs = [s.split("=")[0] for _, switches, _ in mod.cs.SETTINGS for s in switches]
    assert not [k for k in knobs if k in os.environ]              # the record's default rows are those of an empty environment
    got = mod.run_setting("default")
    with open(os.path.join(ROOT, "tests", "golden", "g21_int8_conv_choice.txt")) as fh:
        want = [ln for ln in fh.read().splitlines() if ln.startswith("default | ")]
    assert len(got) == len(want) > 60, (len(got), len(want))
    for a, b in zip(got, want):
        assert a == b
