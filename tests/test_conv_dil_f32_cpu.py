"""The host side of the atrous dense float convolution (fq_conv_dil_f32) on a box without a GPU: the shape decision of
_float_conv (_kd_ok) against the C guard on both sides of every limit, the library-free reference verified() compares the kernel
with, the C ABI's new names, the model, and the kernel's address arithmetic walked by a stand-alone program under the host
sanitizers."""
import os
import re
import subprocess

import pytest
import torch
from torch import nn

from conv_dil_f32_cases import IDS, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kd(cin=16, cout=4, k=3, d=2, **kw):
    if "padding" not in kw:
        kw["padding"] = d if isinstance(d, int) else d[0]
    return nn.Conv2d(cin, cout, k, dilation=d, **kw)


# (name, module, h, w, taken)
GEOMETRIES = [(i, _kd(s[1], s[2], d=s[5], padding=s[6]), s[3], s[4], True) for s, i in zip(SHAPES, IDS)] + [
    ("d 64", _kd(d=64), 9, 11, True),
    ("pad 2d", _kd(d=3, padding=6), 1, 1, True),
    ("plane = span + 1", _kd(d=4, padding=0), 9, 9, True),
    ("d 1", _kd(d=1), 9, 11, False),
    ("d 65", _kd(d=65), 9, 11, False),
    ("pad 2d + 1", _kd(d=2, padding=5), 9, 11, False),
    ("Cin 24", _kd(cin=24), 9, 11, False),
    ("Cout 6", _kd(cout=6), 9, 11, False),
    ("stride 2", _kd(stride=2), 9, 11, False),
    ("5x5", _kd(k=5, padding=4), 19, 19, False),
    ("d (2, 4)", _kd(d=(2, 4), padding=2), 9, 11, False),
    ("plane = span", _kd(d=4, padding=0), 8, 9, False),
]
# what only the Python side can see: these geometries the C guard takes
MODULE_ONLY = [("no bias", _kd(bias=False)), ("circular padding", _kd(padding_mode="circular")), ("string padding", _kd(padding="same"))]


@pytest.mark.parametrize("name,m,h,w,taken", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_kd_ok_is_the_c_guard(name, m, h, w, taken):
    from common.quantity import _float_conv, _native
    assert _float_conv._kd_ok(m, h, w) is taken
    assert _native.conv_dil_f32_supported(m.in_channels, m.out_channels, m.groups, m.kernel_size, m.stride, m.padding, m.dilation,
                                          h, w) is taken


@pytest.mark.parametrize("name,m", MODULE_ONLY, ids=[g[0] for g in MODULE_ONLY])
def test_kd_ok_declines_what_the_c_abi_cannot_see(name, m):
    from common.quantity import _float_conv
    assert not _float_conv._kd_ok(m, 9, 11)


def test_the_switch_is_off_by_default_and_read_at_call_time(monkeypatch):
    from common.quantity import _float_conv
    from tools import pytorch_quantizer
    monkeypatch.delenv("FQ_OWN_DILATED", raising=False)
    assert _float_conv.dilated_enabled() is False and pytorch_quantizer.Quantity.own_dilated is False
    monkeypatch.setenv("FQ_OWN_DILATED", "1")
    assert _float_conv.dilated_enabled() is True
    assert _float_conv.kind(_kd(), torch.zeros(1, 16, 9, 11), dilated=True) is None     # a CPU tensor: there is no CPU path


@pytest.mark.parametrize("shape", SHAPES[:8], ids=IDS[:8])
def test_the_library_free_reference_is_the_convolution(shape):
    from common.quantity import _float_conv
    N, C, K, H, W, d, pad = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(-8, 9, (N, C, H, W), generator=g).float()
    w = torch.randint(-4, 5, (K, C, 3, 3), generator=g).float()
    b = torch.randint(-100, 101, (K,), generator=g).float()
    ref, bound = _float_conv.kd_reference(x, w, b, (d, d), (pad, pad))
    want = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=pad, dilation=d)
    wantb = torch.nn.functional.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=pad, dilation=d)
    assert torch.equal(ref.view_as(want).double(), want) and torch.equal(bound.view_as(want).double(), wantb)


def test_header_declares_the_entry_points_and_the_numerics():
    hdr = open(os.path.join(ROOT, "include", "fq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("fq_conv_dil_f32_supported", "fq_conv_dil_f32", "fq_conv_dil_f32_act", "fq_conv_dil_qd_f32"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
    para = hdr[hdr.index("The atrous dense 3x3 float convolutions"):hdr.index("int fq_conv_dil_f32_supported")]
    assert "acc = fmaf(W[k][c][r][s]" in para and "+0.0f" in para and "NON-FINITE weight" in para
    assert re.search(r"#define FQ_CONV_DIL_F32_CHUNK 8\b", hdr) and re.search(r"#define FQ_VERSION 103\b", hdr)


@pytest.mark.parametrize("output_stride,want", [(16, [2, 2, 6, 12, 18]), (8, [2] * 6 + [4, 4, 12, 24, 36])])
def test_the_model_builds_with_its_dilations(output_stride, want):
    from model.deeplab.DeepLabV3_fabu import DeepLabV3
    model = DeepLabV3(num_classes=5, output_stride=output_stride, width=16, input_size=64).eval()
    convs = [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.dilation[0] > 1]
    assert [m.dilation[0] for m in convs] == want
    assert all(m.kernel_size == (3, 3) and m.groups == 1 and m.in_channels % 16 == 0 and m.padding == m.dilation for m in convs)
    with torch.no_grad():
        assert model(torch.zeros(1, 3, 64, 64)).shape == (1, 5, 64, 64)


def test_the_walker_runs_clean_under_the_host_sanitizers(tmp_path):
    """scripts/conv_dil_f32_geom_check.cpp walks every tile of every launch over the GPU tests' shapes (given as arguments) and,
    without arguments, the DeepLabV3 layers and a padding sweep; it exits non-zero on a staged element from outside x, an LDS read
    outside the staged pixels and the zero pixel, a culled tap with a source inside the image, or an output element written twice
    or not at all."""
    exe = str(tmp_path / "conv_dil_f32_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "scripts", "conv_dil_f32_geom_check.cpp")])
    for args in ([",".join(map(str, s)) for s in SHAPES], []):
        out = subprocess.run([exe] + args, capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.rstrip().splitlines()[-1].startswith("ok,") and not out.stderr, out.stdout + out.stderr
