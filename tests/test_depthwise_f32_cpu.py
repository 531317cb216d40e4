"""The host side of the depthwise float convolution (fq_dwconv_f32) on a box without a GPU: the kernel's address arithmetic walked
by a stand-alone program, the shape decision of _float_conv (_dw_ok / kind), the library-free reference verified() compares the
kernel with, and the C ABI's new symbols."""
import os
import re
import subprocess

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N, C, H, W, R, stride, pad -- the list of tests/test_gpu_depthwise_f32.py
SHAPES = [(1, 1, 1, 1, 3, 1, 1), (2, 3, 3, 3, 3, 1, 0), (1, 5, 4, 6, 5, 1, 4), (3, 7, 7, 7, 3, 1, 1), (2, 19, 14, 14, 3, 2, 1),
          (2, 4, 13, 9, 5, 2, 2), (1, 3, 17, 23, 3, 2, 0), (1, 2, 56, 56, 3, 1, 1), (1, 2, 112, 112, 3, 2, 1), (1, 1, 5, 300, 3, 1, 1),
          (1, 1, 300, 5, 5, 1, 2), (2, 67, 7, 7, 5, 1, 2), (64, 32, 7, 7, 3, 1, 1)]


def test_kernel_address_arithmetic_stays_inside_its_tensors(tmp_path):
    """csrc/fq_dwconv_f32_geom.h holds the kernel's plan and its tile / lane -> address functions and compiles as host code:
    scripts/dwconv_f32_geom_check.cpp walks every lane of every launch over the GPU tests' shapes and MobileNet's layers and
    exits non-zero on a load outside x, an LDS index outside the staged tile, a store outside y, or an output element written
    twice or not at all."""
    exe = str(tmp_path / "dwconv_f32_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "scripts", "dwconv_f32_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,"), out.stdout + out.stderr


def test_the_walkers_shape_list_is_the_gpu_tests():
    src = open(os.path.join(ROOT, "scripts", "dwconv_f32_geom_check.cpp")).read()
    block = src[src.index("const Shape tests[]"):src.index("const Shape net[]")]
    listed = [tuple(int(v) for v in g) for g in re.findall(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}", block)]
    assert listed == SHAPES


def _dw(c=16, k=3, **kw):
    kw.setdefault("groups", c)
    kw.setdefault("padding", 1)
    return nn.Conv2d(c, kw.pop("out", c), k, **kw)


def test_dw_ok_takes_what_the_kernel_takes_and_nothing_else():
    from common.quantity import _float_conv
    for k in (3, 5):
        for stride in (1, 2):
            for pad in range(k):
                assert _float_conv._dw_ok(_dw(k=k, stride=stride, padding=pad), 9, 11), (k, stride, pad)
                assert _float_conv._dw_ok(_dw(k=k, stride=stride, padding=pad), k, k)
    assert _float_conv._dw_ok(_dw(c=1), 1, 1)                                  # a single pixel under a padded 3x3 window
    declined = [
        ("groups 4 of 16", _dw(groups=4)),
        ("depth multiplier 2", _dw(out=32)),
        ("dense", _dw(groups=1)),
        ("dilation 2", _dw(padding=2, dilation=2)),
        ("7x7", _dw(k=7, padding=3)),
        ("1x1", _dw(k=1, padding=0)),
        ("3x5", _dw(k=(3, 5))),
        ("stride (1, 2)", _dw(stride=(1, 2))),
        ("stride 3", _dw(stride=3)),
        ("padding 3 of a 3x3", _dw(padding=3)),
        ("padding 5 of a 5x5", _dw(k=5, padding=5)),
        ("padding (1, 2)", _dw(k=5, padding=(1, 2))),
        ("string padding", _dw(padding="same")),
        ("circular padding", _dw(padding_mode="circular")),
        ("no bias", _dw(bias=False)),
    ]
    for name, m in declined:
        assert not _float_conv._dw_ok(m, 9, 11), name
    assert not _float_conv._dw_ok(_dw(padding=0), 2, 9) and not _float_conv._dw_ok(_dw(k=5, padding=1), 9, 2)   # plane < kernel


def test_kind_is_none_with_the_switch_off_and_never_takes_a_host_tensor(monkeypatch):
    from common.quantity import _float_conv
    monkeypatch.delenv("FQ_OWN_DWCONV", raising=False)
    assert _float_conv.depthwise_enabled() is False                          # the default
    m, x = _dw(), torch.zeros(2, 16, 9, 11)
    assert _float_conv.kind(m, x) is None and _float_conv.kind(m, x, depthwise=False) is None
    assert _float_conv.kind(m, x, depthwise=True) is None                     # a CPU tensor: there is no CPU path
    monkeypatch.setenv("FQ_OWN_DWCONV", "1")
    assert _float_conv.depthwise_enabled() is True                           # read at call time
    monkeypatch.setenv("FQ_OWN_DWCONV", "0")
    assert _float_conv.depthwise_enabled() is False
    from tools import pytorch_quantizer
    assert hasattr(pytorch_quantizer.Quantity, "own_depthwise")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_reference_of_verified_is_a_depthwise_convolution(shape):
    """_float_conv.dw_reference (unfold, products, sum: no convolution library) against F.conv2d(groups=C) in float64: integer-
    valued data exactly, Gaussian data within TOL * bound -- fp32 sums of 9 or 25 terms are off by at most 25 * 2^-24 of
    sum |w||x| whatever their order, an eighth of TOL."""
    from common.quantity import _float_conv
    N, C, H, W, R, stride, pad = shape
    g = torch.Generator().manual_seed(sum(shape))
    for integer in (True, False):
        if integer:
            x = torch.randint(-8, 9, (N, C, H, W), generator=g).float()
            w = torch.randint(-4, 5, (C, 1, R, R), generator=g).float()
            b = torch.randint(-100, 101, (C,), generator=g).float()
        else:
            x, w, b = torch.randn(N, C, H, W, generator=g), torch.randn(C, 1, R, R, generator=g), torch.randn(C, generator=g)
        ref, bound = _float_conv.dw_reference(x, w, b, (R, R), (stride, stride), (pad, pad))
        want = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad, groups=C)
        wantb = torch.nn.functional.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=stride, padding=pad, groups=C)
        assert ref.dtype == torch.float32 and tuple(ref.shape) == (N, C, want.shape[2] * want.shape[3]) and ref.shape == bound.shape
        ref, bound = ref.view_as(want), bound.view_as(want)
        if integer:
            assert torch.equal(ref.double(), want) and torch.equal(bound.double(), wantb)
        else:
            assert bool(((ref.double() - want).abs() <= _float_conv.TOL * wantb).all())
            assert bool(((bound.double() - wantb).abs() <= _float_conv.TOL * wantb).all())


def test_header_declares_the_entry_points_and_the_version_stays():
    hdr = open(os.path.join(ROOT, "include", "fq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("fq_dwconv_f32_supported", "fq_dwconv_f32", "fq_dwconv_qd_f32"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
    assert re.search(r"#define FQ_VERSION 103\b", hdr)
    assert "fmaf(w[r][s], x, acc)" in hdr and "+0.0f" in hdr                  # the numerics paragraph is part of the contract
    from common.quantity import _native
    L = _native.lib()
    assert L.fq_version() == 103
    # host arithmetic only: the answers need no GPU
    assert _native.dwconv_f32_supported(16, (3, 3), (2, 2), (1, 1), (1, 1), 9, 11)
    assert not _native.dwconv_f32_supported(16, (3, 3), (2, 2), (1, 1), (2, 2), 9, 11)
    assert not _native.dwconv_f32_supported(16, (3, 5), (1, 1), (1, 1), (1, 1), 9, 11)
