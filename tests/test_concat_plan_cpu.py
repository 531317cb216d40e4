"""resident.enable(..., concat=True) on a box without a GPU: the tracer, the plan, the handles and the module glue run for real;
the kernel entry points are oracle-backed doubles (tests/native_doubles.py, tests/concat_doubles.py) that follow the reference's
fp32 chain literally.  Every comparison is exact.  The kernel's address arithmetic is walked on the host over the GPU tests'
shape list (scripts/concat_geom_check.cpp)."""
import io
import os
import pickle
import subprocess

import pytest
import torch
from torch import nn

import concat_doubles
import concat_nets as cn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plans(model):
    from common.quantity import resident
    return resident.describe(model)


def _rows(model):
    from common.quantity import resident
    return {n: tuple(getattr(p, f) for f in p.__slots__) for n, p in resident.describe(model).items()}


def _same_outputs(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def _check_forwards(net, x, plain, rows_are_images=True):
    with torch.no_grad():
        assert _same_outputs(net(x), plain)
        if not rows_are_images:                                            # (a Concat along dim 0: the output has 2 N rows)
            return
        assert _same_outputs(net(x[:1]), tuple(p[:1] for p in plain) if isinstance(plain, tuple) else plain[:1])
        flipped = tuple(torch.flip(p, dims=[0]) for p in plain) if isinstance(plain, tuple) else torch.flip(plain, dims=[0])
        assert _same_outputs(net(torch.flip(x, dims=[0])), flipped)


def _default_plan_is_todays(net, x):
    """Without the argument: the branches write fp32 for the Concat (foreign code), no new summary keys, no new forwards."""
    from common.quantity import resident
    a = resident.enable(net, x)
    rows = _rows(net)
    b = resident.enable(net, x, concat=False)
    assert a == b and rows == _rows(net) and set(a) == cn.DEFAULT_KEYS
    plans = _plans(net)
    for name in net.branches:
        assert plans[name].emit_f32, (name, plans[name])
    assert "cat" not in plans and "up" not in plans
    assert "forward" not in net.cat.__dict__
    assert all(p.up is None for p in plans.values())
    resident.disable(net)
    return a


NETS = {
    "fire": (lambda: cn.FireNet(), dict(resident_concats=1, resident_upsamples=0, fused_upsamples=0)),
    "cat_relu": (lambda: cn.CatReluNet(), dict(resident_concats=1, resident_upsamples=0, fused_upsamples=0)),
    "cat_relu_dim_by_name": (lambda: cn.CatReluNet(dim_by_name=True), dict(resident_concats=1, resident_upsamples=0, fused_upsamples=0)),
    "fpn": (lambda: cn.FpnNet(), dict(resident_concats=1, resident_upsamples=1, fused_upsamples=1)),
    "fpn_x4_upsample_module": (lambda: cn.FpnNet(up=nn.Upsample(scale_factor=4, mode="nearest"), factor=4, coarse_c=5),
                               dict(resident_concats=1, resident_upsamples=1, fused_upsamples=1)),
    "fpn_shared": (lambda: cn.FpnNet(shared=True), dict(resident_concats=1, resident_upsamples=1, fused_upsamples=0)),
    "cat_add": (lambda: cn.CatAddNet(), dict(resident_concats=1, resident_upsamples=0, fused_upsamples=0)),
}


@pytest.mark.parametrize("tag", sorted(NETS))
def test_concat_and_upsampling_become_integer_layers(tag):
    from common.quantity import resident
    make, want = NETS[tag]
    with concat_doubles.installed() as nat:
        net, x = make().eval(), cn.example()
        with torch.no_grad():
            plain = net(x)
        assert all(float(p.abs().max()) > 0 for p in (plain if isinstance(plain, tuple) else (plain,)))
        off = _default_plan_is_todays(net, x)

        calls = []
        real = nat.concat_i8_nhwc
        nat.concat_i8_nhwc = lambda srcs, relu, out=None: (calls.append(([(c, u) for _q, c, u in srcs], bool(relu))), real(srcs, relu, out))[1]
        try:
            on = resident.enable(net, x, concat=True)                      # verify=True: bit-identical to the traced forward
            plans = _plans(net)
            assert set(on) == cn.DEFAULT_KEYS | {"resident_concats", "resident_upsamples", "fused_upsamples"}
            assert {k: on[k] for k in want} == want, on
            for name in net.branches:
                assert plans[name].emit_f32 is False and plans[name].emit_int, (name, plans[name])
            assert isinstance(net.cat.__dict__["forward"], resident._ConcatResident)
            assert plans["cat"].emit_int and not plans["cat"].emit_f32 and on["resident_convs"] == off["resident_convs"]
            calls[:] = []
            _check_forwards(net, x, plain)
            per_forward = want["resident_concats"] + want["resident_upsamples"] - want["fused_upsamples"]
            assert len(calls) == 3 * per_forward, calls
            if tag == "fire":
                assert plans["e1"].relu and plans["e3"].relu and not plans["cat"].relu
                assert calls[0] == ([(24, 1), (20, 1)], False)
            if tag.startswith("cat_relu"):
                assert plans["cat"].relu and not plans["branch_a"].relu and calls[0] == ([(8, 1), (8, 1)], True)
                assert plans["add"].resident_add
            if tag == "fpn":
                assert plans["up"].defer and plans["up"].up == 2 and plans["cat"].relu
                assert calls[0] == ([(16, 2), (24, 1)], True)              # the Concat upsamples its first operand itself
            if tag == "fpn_x4_upsample_module":
                assert plans["up"].defer and plans["up"].up == 4 and calls[0] == ([(5, 4), (24, 1)], True)
            if tag == "fpn_shared":
                assert not plans["up"].defer and plans["up"].emit_int and not plans["up"].emit_f32
                assert calls[:2] == [([(16, 2)], False), ([(16, 1), (24, 1)], True)]       # stand-alone upsampling, then the Concat
                assert not plans["coarse"].emit_f32
            if tag == "cat_add":
                assert plans["add"].resident_add and not plans["cat"].relu and plans["add"].relu and on["resident_adds"] == 1
                assert calls[0] == ([(5, 1), (11, 1)], False)
            resident.disable(net)
            assert not _plans(net) and "forward" not in net.cat.__dict__
            assert not hasattr(net, "up") or "forward" not in net.up.__dict__
            calls[:] = []
            with torch.no_grad():
                assert _same_outputs(net(x), plain)
            assert not calls                                               # the default forward again
        finally:
            nat.concat_i8_nhwc = real


DECLINED = {
    "bits_4_and_3": lambda: cn.CatReluNet(bits=(4, 3)),
    "add_sum_as_operand": lambda: cn.CatAddNet(add_operand=True),
    "dim_0": lambda: cn.CatReluNet(dim=0),
    "dim_0_by_name": lambda: cn.CatReluNet(dim=0, dim_by_name=True),
    "scale_factor_3": lambda: cn.FpnNet(up=nn.Upsample(scale_factor=3), factor=3),
    "bilinear": lambda: cn.FpnNet(up=nn.Upsample(scale_factor=2, mode="bilinear")),
    "size_form": lambda: cn.FpnNet(up=nn.Upsample(size=(12, 12))),
}


@pytest.mark.parametrize("tag", sorted(DECLINED))
def test_what_the_plan_declines_stays_in_fp32_form(tag):
    from common.quantity import resident
    with concat_doubles.installed() as nat:
        net, x = DECLINED[tag]().eval(), cn.example()
        with torch.no_grad():
            plain = net(x)
        calls = []
        real = nat.concat_i8_nhwc
        nat.concat_i8_nhwc = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        try:
            on = resident.enable(net, x, concat=True)
            plans = _plans(net)
            if tag in ("scale_factor_3", "bilinear", "size_form"):
                assert on["resident_upsamples"] == 0 and "up" not in plans and "forward" not in net.up.__dict__
                assert plans["coarse"].emit_f32 and on["resident_concats"] == 0 and "cat" not in plans
            else:
                assert on["resident_concats"] == 0 and "cat" not in plans and "forward" not in net.cat.__dict__
                if tag != "add_sum_as_operand":
                    assert all(plans[n].emit_f32 for n in net.branches)
                else:
                    assert plans["add"].emit_f32 and plans["c"].emit_f32
            _check_forwards(net, x, plain, rows_are_images=not tag.startswith("dim_0"))
            assert not calls
        finally:
            nat.concat_i8_nhwc = real


def test_a_deferred_upsample_materialises_for_anything_but_the_concat():
    from common.quantity import resident
    with concat_doubles.installed():
        net, x = cn.FpnNet().eval(), cn.example()
        with torch.no_grad():
            plain = net(x)
            resident.enable(net, x, concat=True)
            s = net.r0(net.stem(x))
            coarse = net.coarse(net.r1(net.down(s)))
            u = net.up(coarse)
            assert type(u) is resident.DeferredUpsample and u.s == 2 and u._out is None and type(coarse) is resident.QHandle
            want = nn.functional.interpolate(coarse.to_f32(), scale_factor=2.0, mode="nearest")
            assert torch.equal(resident.as_f32(u), want)                   # fp32 for foreign code
            h = resident.resident_of(u)                                    # ... and the integer form for an integer layer
            assert type(h) is resident.QHandle and h is u._out and tuple(h.shape) == (4, 16, 12, 12)
            assert h.exact.dtype == torch.int8 and tuple(h.exact.shape) == (4, 12, 12, 16) and h.grid == coarse.grid
            # a materialised operand is then read as an ordinary handle by the Concat, with the same result
            y = net.head(net.r2(net.cat(u, net.fine(s))))
            assert torch.equal(y, plain)
            # a ReLU behind the upsampling is fused into it, and then it is not deferred
            net2 = cn.FpnNet().eval()
            net2.up = nn.Sequential(nn.UpsamplingNearest2d(scale_factor=2), nn.ReLU())
            plain2 = net2(x)
            on = resident.enable(net2, x, concat=True)
            plans = resident.describe(net2)
            assert on["fused_upsamples"] == 0 and on["resident_upsamples"] == 1
            assert plans["up.0"].relu and not plans["up.0"].defer and not plans["up.0"].emit_f32
            assert torch.equal(net2(x), plain2)


def test_a_planned_model_pickles_with_its_plan():
    from common.quantity import resident
    with concat_doubles.installed():
        for make in (cn.FireNet, cn.FpnNet):
            net, x = make().eval(), cn.example()
            with torch.no_grad():
                plain = net(x)
            resident.enable(net, x, concat=True)
            buf = io.BytesIO()
            pickle.dump(net, buf)
            again = pickle.loads(buf.getvalue())
            assert _rows(again) == _rows(net) and isinstance(again.cat.__dict__["forward"], resident._ConcatResident)
            with torch.no_grad():
                assert torch.equal(again(x), plain)
    # a plan pickled before the field `up` existed still loads: __setstate__ starts from __init__
    p = resident.Plan()
    old = {k: v for k, v in p.__getstate__().items() if k != "up"}
    q = resident.Plan.__new__(resident.Plan)
    q.__setstate__(old)
    assert q.up is None and q.__getstate__() == p.__getstate__()


def test_concat_supported_is_host_arithmetic():
    from common.quantity import _native
    assert _native.concat_supported([16, 16], [1, 1]) and _native.concat_supported([3], [4]) and _native.concat_supported([1, 1], [2, 4])
    assert not _native.concat_supported([16, 16], [1, 3]) and not _native.concat_supported([16, 16, 16], [1, 1, 1])
    assert not _native.concat_supported([], []) and not _native.concat_supported([0, 4], [1, 1])
    assert not _native.concat_supported([16], [8]) and not _native.concat_supported([65536, 1], [1, 1])


def test_kernel_address_arithmetic_stays_inside_its_tensors(tmp_path):
    """csrc/fq_concat_i8_geom.h holds the kernel's chunk -> (source, offset, mask) functions and compiles as host code:
    scripts/concat_geom_check.cpp walks every lane of every launch and exits non-zero on a load outside its source, an unaligned
    load, a byte that is not the byte the index rule names, or an output chunk written twice or not at all -- over its built-in
    list and over the GPU tests' shape list."""
    exe = str(tmp_path / "concat_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "scripts", "concat_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,"), out.stdout + out.stderr
    for limit in ("maxsrc=2", "maxsrc=8"):          # the two-source entry point's instantiation, and the N-source one's on the same cases
        out = subprocess.run([exe, limit] + [cn.case_arg(c) for c in cn.KERNEL_CASES], capture_output=True, text=True)
        lines = out.stdout.splitlines()
        assert out.returncode == 0 and lines[-1].startswith("ok,") and len(lines) == len(cn.KERNEL_CASES) + 1, out.stdout + out.stderr
