"""The host side of the atrous depthwise float convolution (fq_dwconv_dil_f32) on a box without a GPU: the shape decision of
_float_conv (_dwd_ok) against the C guard, the library-free reference verified() compares the kernel with, the C ABI's new
names, and the kernel's address arithmetic walked by a stand-alone program under the host sanitizers."""
import os
import re
import subprocess

import pytest
import torch
from torch import nn

from atrous_f32_cases import IDS, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dwd(c=8, k=3, d=2, **kw):
    kw.setdefault("groups", c)
    if "padding" not in kw:
        kw["padding"] = d * (k // 2)
    return nn.Conv2d(c, kw.pop("out", c), k, dilation=d, **kw)


# (name, module, h, w, taken)
GEOMETRIES = [(str(s), _dwd(s[1], s[4], s[5], padding=s[6]), s[2], s[3], True) for s in SHAPES] + [
    ("d 64 5x5", _dwd(k=5, d=64), 9, 11, True),
    ("pad 0, plane = span + 1", _dwd(d=4, padding=0), 9, 9, True),
    ("pad = span", _dwd(d=3, padding=6), 1, 1, True),
    ("d 1", _dwd(d=1), 9, 11, False),
    ("d 65", _dwd(d=65), 9, 11, False),
    ("d (2, 4)", _dwd(d=(2, 4), padding=2), 9, 11, False),
    ("stride 2", _dwd(stride=2), 9, 11, False),
    ("pad > span", _dwd(d=2, padding=5), 9, 11, False),
    ("pad (2, 4)", _dwd(d=2, padding=(2, 4)), 9, 11, False),
    ("7x7", _dwd(k=7), 19, 19, False),
    ("3x5", _dwd(k=(3, 5), padding=2), 19, 19, False),
    ("pad 0, plane = span", _dwd(d=4, padding=0), 8, 9, False),
]
# what only the Python side can see: these geometries the C guard takes
MODULE_ONLY = [("depth multiplier 2", _dwd(out=16)), ("groups 2 of 8", _dwd(groups=2)), ("dense", _dwd(groups=1)),
               ("no bias", _dwd(bias=False)), ("circular padding", _dwd(padding_mode="circular")),
               ("string padding", _dwd(padding="same"))]


@pytest.mark.parametrize("name,m,h,w,taken", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_dwd_ok_is_the_c_guard(name, m, h, w, taken):
    from common.quantity import _float_conv, _native
    assert _float_conv._dwd_ok(m, h, w) is taken
    assert _native.dwconv_dil_f32_supported(m.in_channels, m.kernel_size, m.stride, m.padding, m.dilation, h, w) is taken


@pytest.mark.parametrize("name,m", MODULE_ONLY, ids=[g[0] for g in MODULE_ONLY])
def test_dwd_ok_declines_what_the_c_abi_cannot_see(name, m):
    from common.quantity import _float_conv
    assert not _float_conv._dwd_ok(m, 9, 11)


def test_the_switch_is_off_by_default_and_read_at_call_time(monkeypatch):
    from common.quantity import _float_conv
    from tools import pytorch_quantizer
    monkeypatch.delenv("FQ_OWN_ATROUS", raising=False)
    assert _float_conv.atrous_enabled() is False and pytorch_quantizer.Quantity.own_atrous is False
    monkeypatch.setenv("FQ_OWN_ATROUS", "1")
    assert _float_conv.atrous_enabled() is True
    assert _float_conv.kind(_dwd(), torch.zeros(1, 8, 9, 11), atrous=True) is None      # a CPU tensor: there is no CPU path


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_reference_of_verified_takes_a_dilation(shape):
    from common.quantity import _float_conv
    N, C, H, W, R, d, pad = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(-8, 9, (N, C, H, W), generator=g).float()
    w = torch.randint(-4, 5, (C, 1, R, R), generator=g).float()
    b = torch.randint(-100, 101, (C,), generator=g).float()
    ref, bound = _float_conv.dw_reference(x, w, b, (R, R), (1, 1), (pad, pad), dilation=d)
    want = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=pad, dilation=d, groups=C)
    wantb = torch.nn.functional.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=pad, dilation=d, groups=C)
    assert torch.equal(ref.view_as(want).double(), want) and torch.equal(bound.view_as(want).double(), wantb)


def test_header_declares_the_entry_points_and_the_numerics():
    hdr = open(os.path.join(ROOT, "include", "fq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("fq_dwconv_dil_f32_supported", "fq_dwconv_dil_f32", "fq_dwconv_dil_f32_act", "fq_dwconv_dil_qd_f32"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
    para = hdr[hdr.index("The atrous depthwise float convolutions"):hdr.index("int fq_dwconv_dil_f32_supported")]
    assert "fmaf(w[r][s], x, acc)" in para and "+0.0f" in para and "never a masked product" in para
    assert re.search(r"#define FQ_VERSION 103\b", hdr)


def test_the_walker_has_the_shape_list_and_runs_clean_under_the_host_sanitizers(tmp_path):
    """scripts/dwconv_dil_f32_geom_check.cpp walks every lane of every launch over this list and the DeepLabV3+ layers and exits
    non-zero on a staged element from outside x, an LDS read outside the staged rows and the zero row, or an output element
    written twice or not at all."""
    path = os.path.join(ROOT, "scripts", "dwconv_dil_f32_geom_check.cpp")
    src = open(path).read()
    block = src[src.index("const Shape tests[]"):src.index("const Shape net[]")]
    listed = [tuple(int(v) for v in g) for g in re.findall(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}", block)]
    assert listed == SHAPES
    exe = str(tmp_path / "dwconv_dil_f32_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, path])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,") and not out.stderr, out.stdout + out.stderr
