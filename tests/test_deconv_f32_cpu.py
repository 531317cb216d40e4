"""The host side of the transposed float convolution (fq_deconv_f32) on a box without a GPU: the kernel's address arithmetic walked
by a stand-alone program under the sanitizers, the shape decision of the C ABI and of _float_conv.kind, the cached weight pack, the
library-free reference verified() compares the kernel with, an emulator of the numerics contract (the fmaf chain of include/fq.h,
with libm's fmaf), and the header's text."""
import os
import re
import subprocess

import pytest
import torch
from torch import nn

from deconv_f32_util import (BIG, CONTRACT_IDS, CONTRACT_LIMIT, CONTRACT_SHAPES, IDS, ROOT, SHAPES, emulate, macs, max_blocks, operands,
                             out_hw, pack, ref64, work_items)


def test_header_declares_the_entry_points_and_the_numerics_and_the_version_stays():
    hdr = open(os.path.join(ROOT, "include", "fq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("fq_deconv_f32_supported", "fq_deconv_f32"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
    assert re.search(r"#define FQ_VERSION 103\b", hdr)
    text = re.sub(r"\n \*", "\n", hdr)                                       # the comment's left margin
    flat = re.sub(r"\s+", " ", text)
    for line in ("acc = +0.0f",
                 "for r ascending with (oh + pad - r) % stride == 0:",
                 "for s ascending with (ow + pad - s) % stride == 0:",
                 "for c in 0 .. Cin-1:",
                 "acc = fmaf(w[c][k][r][s], x[n][c][(oh + pad - r)/stride][(ow + pad - s)/stride], acc)",
                 "y = acc + bias[k] (bias == NULL: acc + 0.0f)",
                 "A tap whose source pixel lies outside the image is the operand +0.0f.",
                 "It is never a value loaded from a neighbouring row or plane.",
                 "An output with no tap at all (kernel smaller than stride) is +0.0f + bias[k].",
                 "There is no K split, no workspace, and no float atomics other than the abs-max publish.",
                 "The value depends on neither N nor the tile, lane or code path.",
                 "Image i of a batch gets the bits of the same image alone.",
                 "Exact zeros are not counted by the histogram.",
                 "The abs-max ignores NaN."):
        assert line in flat, line
    from common.quantity import _native
    assert _native.lib().fq_version() == 103


def test_supported_answers_on_the_host():
    from common.quantity import _native

    def sup(cin=16, cout=4, groups=1, k=(3, 3), stride=(2, 2), pad=(1, 1), outpad=(1, 1), dil=(1, 1), h=5, w=7):
        return _native.deconv_f32_supported(cin, cout, groups, k, stride, pad, outpad, dil, h, w)

    for (_N, cin, cout, H, W, R, S, stride, pad, outpad) in SHAPES:
        assert sup(cin, cout, 1, (R, S), (stride, stride), (pad, pad), (outpad, outpad), (1, 1), H, W), (cin, cout, H, W, R, S)
    assert sup()
    declined = [("groups 2", dict(groups=2)), ("dilation 2", dict(dil=(2, 2))), ("Cin 24", dict(cin=24)), ("Cout 6", dict(cout=6)),
                ("kernel 9", dict(k=(9, 9))), ("stride 5", dict(stride=(5, 5))), ("stride 1x2", dict(stride=(1, 2))),
                ("pad == R", dict(pad=(3, 3))), ("outpad == stride", dict(outpad=(2, 2)))]
    for name, kw in declined:
        assert not sup(**kw), name
    # ... and the neighbours of those limits that are taken
    assert sup(k=(8, 8), pad=(7, 7)) and sup(stride=(4, 4), outpad=(3, 3)) and sup(cin=32, cout=8) and sup(pad=(2, 2))
    assert not sup(pad=(1, 2)) and not sup(outpad=(0, 1)) and not sup(k=(3, 2), pad=(2, 2)) and not sup(cin=0) and not sup(h=0)
    assert not sup(k=(1, 1), stride=(1, 1), pad=(0, 0), outpad=(0, 0), h=0, w=3)


def test_the_geometry_program_passes_under_the_sanitizers(tmp_path):
    """csrc/fq_deconv_f32_geom.h holds the kernel's plan and its work-item / lane -> address functions and compiles as host code:
    scripts/deconv_f32_geom_check.cpp walks every lane of every launch over the GPU tests' shapes and the U-Net's up-convolutions
    and exits non-zero on a load outside x or wt, a store outside y, an output element written twice or not at all, or a tap that
    is not the definition's.  Built with AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program."""
    exe = str(tmp_path / "deconv_f32_geom_check")
    subprocess.check_call(["c++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "scripts", "deconv_f32_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,"), out.stdout + out.stderr


def test_the_walkers_shape_list_is_the_gpu_tests_and_one_launch_exceeds_the_largest_grid():
    src = open(os.path.join(ROOT, "scripts", "deconv_f32_geom_check.cpp")).read()
    block = src[src.index("const Shape tests[]"):src.index("const Shape net[]")]
    listed = [tuple(int(v) for v in g) for g in re.findall(r"\{" + ", ".join([r"(\d+)"] * 10) + r"\}", block)]
    assert listed == SHAPES
    import test_gpu_deconv_f32
    assert test_gpu_deconv_f32.SHAPES is SHAPES                               # one list, in tests/deconv_f32_util.py
    assert SHAPES[-1] == BIG and work_items(BIG) > max_blocks() >= 1024
    assert all(macs(s) < CONTRACT_LIMIT for s in CONTRACT_SHAPES) and len(CONTRACT_SHAPES) == 11


def test_makefile_names_both_files():
    mk = open(os.path.join(ROOT, "pytorch-quantity_amd", "csrc", "Makefile")).read()
    srcs = mk[mk.index("SRCS :="):mk.index("HDRS :=")]
    hdrs = mk[mk.index("HDRS :="):mk.index("FLAGS :=")]
    assert "fq_deconv_f32.hip" in srcs.split() and "fq_deconv_f32_geom.h" in hdrs.split()


@pytest.mark.parametrize("shape", CONTRACT_SHAPES, ids=CONTRACT_IDS)
def test_the_contract_emulator_is_a_transposed_convolution(shape):
    """The fmaf chain of include/fq.h, evaluated with libm's fmaf: exact on integer-valued data, within TOL * bound of float64 on
    Gaussian data (a chain of n fmaf roundings is off by at most n * 2^-24 of sum |w||x|; n <= Cin * taps = 48 * 4 here, a
    thousandth of TOL's 1e-5)."""
    from common.quantity import _float_conv
    _N, cin, _cout, _H, _W, R, S, stride, pad, outpad = shape
    assert macs(shape) < CONTRACT_LIMIT
    # integer operands are at most 8 and 4 in magnitude, the bias at most 100: every partial sum is an integer below 2^24
    assert cin * -(-R // stride) * -(-S // stride) * 32 + 100 < 2 ** 24
    x, w, b = operands(shape, True)
    assert torch.equal(emulate(x, w, b, stride, pad, outpad).double(), ref64(x, w, b, stride, pad, outpad))
    x, w, b = operands(shape, False)
    y = emulate(x, w, b, stride, pad, outpad)
    want, bound = ref64(x, w, b, stride, pad, outpad), ref64(x.abs(), w.abs(), b.abs(), stride, pad, outpad)
    assert tuple(y.shape[2:]) == out_hw(shape) and bool(((y.double() - want).abs() <= _float_conv.TOL * bound).all())
    dref, dbound = _float_conv.dc_reference(x, w, b, (R, S), (stride, stride), (pad, pad), (outpad, outpad))
    assert bool(((y - dref).abs() <= _float_conv.TOL * dbound).all())        # ... and of the reference verified() holds the kernel to
    if macs(shape) < 20000:                                                 # no bias: acc + 0.0f
        y0 = emulate(x, w, None, stride, pad, outpad)
        assert bool(((y0.double() - ref64(x, w, None, stride, pad, outpad)).abs()
                     <= _float_conv.TOL * ref64(x.abs(), w.abs(), None, stride, pad, outpad)).all())


@pytest.mark.parametrize("shape", CONTRACT_SHAPES, ids=CONTRACT_IDS)
def test_the_reference_of_verified_is_a_transposed_convolution(shape):
    """_float_conv.dc_reference (one matmul, F.fold, the bias: no convolution library) against F.conv_transpose2d in float64:
    integer-valued data exactly, Gaussian data within TOL * bound."""
    from common.quantity import _float_conv
    N, _cin, cout, _H, _W, R, S, stride, pad, outpad = shape
    for integer in (True, False):
        x, w, b = operands(shape, integer)
        ref, bound = _float_conv.dc_reference(x, w, b, (R, S), (stride, stride), (pad, pad), (outpad, outpad))
        want = ref64(x, w, b, stride, pad, outpad)
        wantb = ref64(x.abs(), w.abs(), b.abs(), stride, pad, outpad)
        assert ref.dtype == torch.float32 and tuple(ref.shape) == (N, cout) + out_hw(shape) and ref.shape == bound.shape
        f32 = torch.nn.functional.conv_transpose2d(x, w, b, stride=stride, padding=pad, output_padding=outpad)
        if integer:
            assert float(wantb.max()) < 2 ** 24
            assert torch.equal(ref.double(), want) and torch.equal(bound.double(), wantb) and torch.equal(ref, f32)
        else:
            assert bool(((ref.double() - want).abs() <= _float_conv.TOL * wantb).all())
            assert bool(((bound.double() - wantb).abs() <= _float_conv.TOL * wantb).all())
            assert bool(((ref - f32).abs().double() <= _float_conv.TOL * wantb).all())


class FakeCuda(torch.Tensor):
    is_cuda = True


def _dc(cin=16, cout=8, k=3, **kw):
    kw.setdefault("stride", 2)
    kw.setdefault("padding", 1)
    kw.setdefault("output_padding", 1)
    return nn.ConvTranspose2d(cin, cout, k, **kw)


def test_kind_takes_a_qualifying_layer_only_with_the_switch_on(monkeypatch):
    """kind() on tensors that claim to be CUDA fp32 (no GPU here: the guards read attributes only)."""
    from common.quantity import _float_conv
    from tools import pytorch_quantizer
    monkeypatch.delenv("FQ_OWN_DECONV", raising=False)
    assert _float_conv.deconv_enabled() is False                            # the default
    assert pytorch_quantizer.Quantity.own_deconv is False and hasattr(pytorch_quantizer.Quantity, "own_grouped")
    m = _dc()
    x = torch.zeros(2, 16, 5, 7).as_subclass(FakeCuda)
    assert _float_conv.kind(m, x) is None and _float_conv.kind(m, x, deconv=False) is None
    assert _float_conv.kind(m, x, deconv=True) == "dc"
    assert _float_conv.kind(m, torch.zeros(2, 16, 5, 7), deconv=True) is None      # a CPU tensor: there is no CPU path
    assert _float_conv.kind(m, x, depthwise=True, grouped=True) is None            # the other switches do not open it
    assert _float_conv.kind(_dc(bias=False), x, deconv=True) is None
    circ = _dc()
    circ.padding_mode = "circular"                                          # (the constructor refuses it: set as a foreign model might)
    assert _float_conv.kind(circ, x, deconv=True) is None
    assert _float_conv.kind(m, x.double(), deconv=True) is None
    assert _float_conv.kind(m, x.transpose(2, 3), deconv=True) is None      # not contiguous
    from common.quantity import _native

    def abi(mod, h=5, w=7):
        """what fq_deconv_f32_supported answers for the module's own numbers: kind() keeps a second copy of those limits"""
        return _native.deconv_f32_supported(mod.in_channels, mod.out_channels, mod.groups, mod.kernel_size, mod.stride, mod.padding,
                                            mod.output_padding, mod.dilation, h, w)

    bad24 = _dc(cin=24)
    for name, bad in (("groups 2", _dc(groups=2)), ("dilation 2", _dc(dilation=2)), ("Cout 6", _dc(cout=6)), ("kernel 9", _dc(k=9)),
                      ("stride 5", _dc(stride=5)), ("stride 1x2", _dc(stride=(1, 2), output_padding=0)),
                      ("outpad 0x1", _dc(output_padding=(0, 1))), ("pad 1x2", _dc(padding=(1, 2))),
                      ("pad == R", _dc(k=3, padding=3, output_padding=0)), ("Cin 24", bad24)):
        xin = torch.zeros(2, bad.in_channels, 5, 7).as_subclass(FakeCuda)
        assert _float_conv.kind(bad, xin, deconv=True) is None, name
        assert not abi(bad), name                                            # the C ABI declines the same geometry
    for k_, st, p, op in ((2, 2, 0, 0), (4, 2, 1, 0), (8, 4, 7, 3), (1, 2, 0, 1), (3, 1, 1, 0), ((2, 3), 3, 1, 2), (3, 4, 2, 3),
                          ((8, 1), 2, 0, 1)):
        good = _dc(k=k_, stride=st, padding=p, output_padding=op)
        assert _float_conv.kind(good, x, deconv=True) == "dc", (k_, st, p, op)
        assert abi(good), (k_, st, p, op)
    # a plane that leaves no output: both decline
    tiny = _dc(k=1, stride=1, padding=0, output_padding=0)
    assert abi(tiny, 1, 1) and _float_conv.kind(tiny, torch.zeros(1, 16, 1, 1).as_subclass(FakeCuda), deconv=True) == "dc"
    gone = _dc(k=(2, 2), stride=1, padding=1, output_padding=0)                # Ho = H - 1 + 2 - 2 = H - 1: nothing left of one row
    assert not abi(gone, 1, 7) and _float_conv.kind(gone, torch.zeros(1, 16, 1, 7).as_subclass(FakeCuda), deconv=True) is None

    class Sub(nn.ConvTranspose2d):
        pass
    assert _float_conv.kind(Sub(16, 8, 2, stride=2), x, deconv=True) is None       # `type(m) is`: a subclass may override forward
    monkeypatch.setenv("FQ_OWN_DECONV", "1")
    assert _float_conv.deconv_enabled() is True and _float_conv.kind(m, x) == "dc" and _float_conv.kind(m, x, deconv=False) is None
    assert _float_conv.kind(nn.Conv2d(16, 8, 3, padding=1), x) == "kxk"      # an ordinary convolution is what it was
    monkeypatch.setenv("FQ_OWN_DECONV", "0")
    assert _float_conv.deconv_enabled() is False and _float_conv.kind(m, x) is None
    assert _float_conv.kernel_key(m, "dc") == ("dc", False)
    assert "deconv_enabled" in _float_conv.__all__ and "dc_reference" in _float_conv.__all__
    assert not any(k_.startswith("_fq") or "fq" in k_ for k_ in m.__dict__)  # nothing is stored on the module


def test_weight_is_the_stated_layout_and_follows_the_parameter():
    from common.quantity import _float_conv
    m = nn.ConvTranspose2d(16, 8, (2, 3), stride=3)
    w = m.weight.detach()
    wt = _float_conv.weight(m, "dc")
    assert tuple(wt.shape) == (2 * 3 * 16, 8) and wt.is_contiguous() and torch.equal(wt, pack(w))
    for r in range(2):
        for s in range(3):
            for c in range(16):
                for k in range(8):
                    assert float(wt[(r * 3 + s) * 16 + c, k]) == float(w[c, k, r, s])
    assert _float_conv.weight(m, "dc") is wt                                 # cached
    with torch.no_grad():
        m.weight.mul_(2.0)                                                   # written in place: re-made
    wt2 = _float_conv.weight(m, "dc")
    assert wt2 is not wt and torch.equal(wt2, pack(m.weight.detach()))
    m.weight = nn.Parameter(torch.ones_like(m.weight))                       # replaced: re-made
    assert torch.equal(_float_conv.weight(m, "dc"), torch.ones(96, 8))
    assert "forward" not in m.__dict__ and set(m.__dict__) == set(nn.ConvTranspose2d(16, 8, (2, 3), stride=3).__dict__)
    _float_conv.forget(m)
