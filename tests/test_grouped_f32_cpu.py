"""The host side of the grouped float convolution (fq_gconv_f32) on a box without a GPU: the kernel's address arithmetic walked by a
stand-alone program, the shape decision of _float_conv (_g_ok / kind), the library-free reference verified() compares the kernel
with, an emulator of the numerics contract (the fmaf chain of include/fq.h, with libm's fmaf), and the C ABI's new symbols."""
import os
import re
import subprocess

import pytest
import torch
from torch import nn

from grouped_f32_util import CONTRACT_SHAPES, IDS, SHAPES, emulate, macs, operands, ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_address_arithmetic_stays_inside_its_tensors(tmp_path):
    """csrc/fq_gconv_f32_geom.h holds the kernel's plan and its tile / lane -> address functions and compiles as host code:
    scripts/gconv_f32_geom_check.cpp walks every lane of every launch over the GPU tests' shapes and ResNeXt-50's layers and
    exits non-zero on a load outside x or w, an LDS index outside the staged tile, a tap that reads another pixel's or weight's
    LDS float, a store outside y, an output element written twice or not at all, or a reciprocal division that is off."""
    exe = str(tmp_path / "gconv_f32_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "scripts", "gconv_f32_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,"), out.stdout + out.stderr


def test_the_walkers_shape_list_is_the_gpu_tests():
    src = open(os.path.join(ROOT, "scripts", "gconv_f32_geom_check.cpp")).read()
    block = src[src.index("const Shape tests[]"):src.index("const Shape net[]")]
    listed = [tuple(int(v) for v in g) for g in re.findall(r"\{" + ", ".join([r"(\d+)"] * 9) + r"\}", block)]
    assert listed == SHAPES
    import test_gpu_grouped_f32
    assert test_gpu_grouped_f32.SHAPES is SHAPES                              # one list, in tests/grouped_f32_util.py
    net = src[src.index("const Shape net[]"):src.index("long total = 0;")]
    assert len(re.findall(r"\{1, 32, ", net)) == 16                           # ResNeXt-50's sixteen grouped layers


def _g(c=16, out=None, k=3, groups=2, **kw):
    kw.setdefault("padding", 1 if k == 3 else 0)
    return nn.Conv2d(c, c if out is None else out, k, groups=groups, **kw)


def test_g_ok_takes_what_the_kernel_takes_and_nothing_else():
    from common.quantity import _float_conv
    for k in (1, 3):
        for stride in (1, 2):
            for pad in range(k):
                assert _float_conv._g_ok(_g(k=k, stride=stride, padding=pad), 9, 11), (k, stride, pad)
                assert _float_conv._g_ok(_g(k=k, stride=stride, padding=pad), k, k)
    assert _float_conv._g_ok(_g(c=16, out=32, groups=4), 9, 11)                # 4 -> 8 per group
    assert _float_conv._g_ok(_g(c=24, out=8, groups=2), 9, 11)                 # 12 -> 4
    assert _float_conv._g_ok(_g(c=8, groups=2), 1, 1)                          # 4 per group; a single pixel under a padded window
    assert _float_conv._g_ok(_g(c=128, groups=2), 9, 11)                       # 64 per group
    assert _float_conv._g_ok(_g(c=128, out=8, groups=2), 9, 11) and _float_conv._g_ok(_g(c=8, out=128, groups=2), 9, 11)
    declined = [
        ("depthwise", _g(groups=16)),
        ("depth multiplier 2", _g(out=32, groups=16)),
        ("dense", _g(groups=1)),
        ("2 per group", _g(c=16, groups=8)),
        ("2 output channels per group", _g(c=16, out=8, groups=4)),
        ("6 per group", _g(c=12, groups=2)),
        ("68 per group", _g(c=136, groups=2)),
        ("68 output channels per group", _g(c=16, out=136, groups=2)),
        ("dilation 2", _g(padding=2, dilation=2)),
        ("5x5", _g(k=5, padding=2)),
        ("3x1", _g(k=(3, 1), padding=0)),
        ("stride (1, 2)", _g(stride=(1, 2))),
        ("stride 3", _g(stride=3)),
        ("padding 3 of a 3x3", _g(padding=3)),
        ("padding 1 of a 1x1", _g(k=1, padding=1)),
        ("padding (1, 2)", _g(padding=(1, 2))),
        ("string padding", _g(padding="same")),
        ("circular padding", _g(padding_mode="circular")),
        ("no bias", _g(bias=False)),
    ]
    for name, m in declined:
        assert not _float_conv._g_ok(m, 9, 11), name
    assert not _float_conv._g_ok(_g(padding=0), 2, 9) and not _float_conv._g_ok(_g(padding=0), 9, 2)   # plane < kernel
    # the C ABI answers the same for the same numbers (host arithmetic: no GPU needed)
    from common.quantity import _native
    for name, m in declined[:-3] + [("ok", _g()), ("ok 1x1/2", _g(k=1, stride=2)), ("ok 4->8", _g(c=16, out=32, groups=4))]:
        if isinstance(m.padding, str):
            continue
        want = _float_conv._g_ok(m, 9, 11)
        assert _native.gconv_f32_supported(m.in_channels, m.out_channels, m.groups, m.kernel_size, m.stride, m.padding, m.dilation,
                                           9, 11) == want, name
    assert not _native.gconv_f32_supported(16, 16, 2, (3, 3), (1, 1), (0, 0), (1, 1), 2, 9)


def test_kind_is_none_with_the_switch_off_and_never_takes_a_host_tensor(monkeypatch):
    from common.quantity import _float_conv
    monkeypatch.delenv("FQ_OWN_GCONV", raising=False)
    monkeypatch.delenv("FQ_OWN_DWCONV", raising=False)
    assert _float_conv.grouped_enabled() is False                            # the default
    m, x = _g(), torch.zeros(2, 16, 9, 11)
    assert _float_conv.kind(m, x) is None and _float_conv.kind(m, x, grouped=False) is None
    assert _float_conv.kind(m, x, grouped=True) is None                       # a CPU tensor: there is no CPU path
    monkeypatch.setenv("FQ_OWN_GCONV", "1")
    assert _float_conv.grouped_enabled() is True                             # read at call time
    monkeypatch.setenv("FQ_OWN_GCONV", "0")
    assert _float_conv.grouped_enabled() is False
    from tools import pytorch_quantizer
    assert pytorch_quantizer.Quantity.own_grouped is False and hasattr(pytorch_quantizer.Quantity, "own_depthwise")


def test_kind_keeps_depthwise_and_grouped_layers_apart(monkeypatch):
    """kind() on tensors that claim to be CUDA fp32 (no GPU here: the guards read attributes only): "g" needs the grouped
    switch, "dw" the depthwise switch, whatever the other says; everything else is what it was."""
    from common.quantity import _float_conv
    monkeypatch.delenv("FQ_OWN_GCONV", raising=False)
    monkeypatch.delenv("FQ_OWN_DWCONV", raising=False)

    class FakeCuda(torch.Tensor):
        is_cuda = True

    x = torch.zeros(2, 16, 9, 11).as_subclass(FakeCuda)
    g, dw = _g(), _g(groups=16)
    assert _float_conv.kind(g, x) is None and _float_conv.kind(dw, x) is None
    assert _float_conv.kind(g, x, grouped=True) == "g" and _float_conv.kind(g, x, depthwise=True) is None
    assert _float_conv.kind(g, x, depthwise=True, grouped=False) is None
    assert _float_conv.kind(dw, x, grouped=True) is None and _float_conv.kind(dw, x, depthwise=True) == "dw"
    assert _float_conv.kind(dw, x, depthwise=True, grouped=True) == "dw" and _float_conv.kind(dw, x, depthwise=False, grouped=True) is None
    monkeypatch.setenv("FQ_OWN_GCONV", "1")
    assert _float_conv.kind(g, x) == "g" and _float_conv.kind(dw, x) is None and _float_conv.kind(g, x, grouped=False) is None
    assert _float_conv.kind(_g(c=12, groups=2), torch.zeros(2, 12, 9, 11).as_subclass(FakeCuda), grouped=True) is None     # 6 per group: declined with the switch on
    assert _float_conv.kind(_g(bias=False), x, grouped=True) is None
    monkeypatch.setenv("FQ_OWN_DWCONV", "1")
    assert _float_conv.kind(g, x) == "g" and _float_conv.kind(dw, x) == "dw"
    monkeypatch.setenv("FQ_OWN_GCONV", "0")
    assert _float_conv.kind(g, x) is None and _float_conv.kind(dw, x) == "dw"
    assert _float_conv.kernel_key(g, "g") == ("g", False)
    assert _float_conv.weight(g, "g").data_ptr() == g.weight.data_ptr()       # the module's own layout: no pack, no cache entry
    assert "wt" not in _float_conv.state(g)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_reference_of_verified_is_a_grouped_convolution(shape):
    """_float_conv.g_reference (unfold, one batched matmul over the groups: no convolution library) against F.conv2d(groups=G) in
    float64: integer-valued data exactly, Gaussian data within TOL * bound -- an fp32 sum of n <= 577 terms is off by at most
    n * 2^-24 of sum |w||x| whatever its order, a third of TOL."""
    from common.quantity import _float_conv
    N, G, cgi, cgo, H, W, R, stride, pad = shape
    for integer in (True, False):
        x, w, b = operands(shape, integer)
        ref, bound = _float_conv.g_reference(x, w, b, G, (R, R), (stride, stride), (pad, pad))
        want = ref64(x, w, b, G, stride, pad)
        wantb = ref64(x.abs(), w.abs(), b.abs(), G, stride, pad)
        assert ref.dtype == torch.float32 and tuple(ref.shape) == (N, G * cgo, want.shape[2] * want.shape[3]) and ref.shape == bound.shape
        ref, bound = ref.view_as(want), bound.view_as(want)
        if integer:
            assert float(wantb.max()) < 2 ** 24
            assert torch.equal(ref.double(), want) and torch.equal(bound.double(), wantb)
        else:
            assert bool(((ref.double() - want).abs() <= _float_conv.TOL * wantb).all())
            assert bool(((bound.double() - wantb).abs() <= _float_conv.TOL * wantb).all())


@pytest.mark.parametrize("shape", CONTRACT_SHAPES, ids=["x".join(map(str, s)) for s in CONTRACT_SHAPES])
def test_the_contract_emulator_is_a_grouped_convolution(shape):
    """The fmaf chain of include/fq.h, evaluated with libm's fmaf: exact on integer-valued data, within TOL * bound of float64 on
    Gaussian data (a chain of n fmaf roundings is off by at most n * 2^-24 of sum |w||x|)."""
    from common.quantity import _float_conv
    _N, G, _cgi, _cgo, _H, _W, _R, stride, pad = shape
    assert macs(shape) < 500000
    x, w, b = operands(shape, True)
    assert torch.equal(emulate(x, w, b, G, stride, pad).double(), ref64(x, w, b, G, stride, pad))
    x, w, b = operands(shape, False)
    y = emulate(x, w, b, G, stride, pad)
    assert bool(((y.double() - ref64(x, w, b, G, stride, pad)).abs() <= _float_conv.TOL * ref64(x.abs(), w.abs(), b.abs(), G, stride, pad)).all())
    R = shape[6]                                                             # and of the reference verified() holds the kernel to
    gref, gbound = _float_conv.g_reference(x, w, b, G, (R, R), (stride, stride), (pad, pad))
    assert bool(((y.view(gref.shape) - gref).abs() <= _float_conv.TOL * gbound).all())
    if macs(shape) < 20000:                                                  # no bias: acc + 0.0f
        y0 = emulate(x, w, None, G, stride, pad)
        assert bool(((y0.double() - ref64(x, w, None, G, stride, pad)).abs()
                     <= _float_conv.TOL * ref64(x.abs(), w.abs(), None, G, stride, pad)).all())


def test_the_contract_shapes_reach_every_instantiation_and_tiling():
    """Which shapes the contract test can afford: every <R, stride> instantiation of the kernel, a group whose output channels
    go in more than one chunk, more than one column block, more than one row band."""
    fams = {(s[6], s[7]) for s in CONTRACT_SHAPES}
    assert fams == {(1, 1), (1, 2), (3, 1), (3, 2)}
    assert (1, 2, 64, 40, 3, 3, 3, 1, 1) in CONTRACT_SHAPES and (1, 2, 4, 4, 3, 70, 3, 1, 1) in CONTRACT_SHAPES
    assert (1, 2, 64, 4, 24, 3, 3, 1, 1) in CONTRACT_SHAPES
    # and the list holds a launch with more tiles than the largest grid has workgroups (one tile per image and group there)
    geom = open(os.path.join(ROOT, "pytorch-quantity_amd", "csrc", "fq_gconv_f32_geom.h")).read()
    cap = int(re.search(r"constexpr int kGfMaxBlocks = (\d+);", geom).group(1))
    assert (33, 64, 4, 4, 7, 7, 3, 1, 1) in SHAPES and 33 * 64 > cap


def test_header_declares_the_entry_points_and_the_version_stays():
    hdr = open(os.path.join(ROOT, "include", "fq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("fq_gconv_f32_supported", "fq_gconv_f32", "fq_gconv_qd_f32"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
    assert re.search(r"#define FQ_VERSION 103\b", hdr)
    # the numerics paragraph is part of the contract
    assert "acc = fmaf(w[k][c][r][s], x[n][g*Cgi + c][oh*stride - pad + r][ow*stride - pad + s], acc)" in hdr
    assert "for r: for s: for c in 0 .. Cgi-1:" in hdr and "acc = +0.0f" in hdr and "y = acc + bias[k]" in hdr
    from common.quantity import _native
    L = _native.lib()
    assert L.fq_version() == 103
    # host arithmetic only: the answers need no GPU
    assert _native.gconv_f32_supported(16, 32, 4, (3, 3), (2, 2), (1, 1), (1, 1), 9, 11)
    assert not _native.gconv_f32_supported(16, 32, 4, (3, 3), (2, 2), (1, 1), (2, 2), 9, 11)
    assert not _native.gconv_f32_supported(16, 16, 16, (3, 3), (1, 1), (1, 1), (1, 1), 9, 11)
    assert not _native.gconv_f32_supported(16, 16, 1, (3, 3), (1, 1), (1, 1), (1, 1), 9, 11)
