"""resident.enable(..., depthwise=True) and NewConv2d.use_depthwise_i8 on a box without a GPU: the tracer, the plan, the handles
and the module glue run for real; the kernel entry points are oracle-backed doubles (tests/native_doubles.py,
tests/depthwise_doubles.py) that follow the reference's fp32 chain literally.  Every comparison is exact."""
import io
import pickle

import pytest
import torch
from torch import nn

import cases
import depthwise_doubles
import depthwise_nets as dn

PLAN_FIELDS = ("relu", "emit_f32", "emit_int", "narrow_bit", "want_wide", "grid", "resident_add", "defer", "fuse_arg",
               "fuse_next", "narrow_to_hbm", "fuse_proj", "depthwise")


def _tiny(per_channel=False):
    model = dn.seeded(cases.tiny_separable_net().eval())
    info = dn.fixed_info(model, per_channel=per_channel)
    return dn.rebuild(model, info), info, torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(1))


def _add_net(per_channel=False):
    model = dn.seeded(dn.SeparableAddNet().eval(), seed=5)
    info = dn.fixed_info(model, per_channel=per_channel, seed=2)
    return dn.rebuild(model, info), info, torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(2))


def _plan_rows(model):
    from common.quantity import resident
    return {name: tuple(getattr(p, f) for f in PLAN_FIELDS) for name, p in resident.describe(model).items()}


@pytest.mark.parametrize("per_channel", [False, "depthwise"])
def test_depthwise_layers_of_a_separable_net_become_integer_layers(per_channel):
    from common.quantity import resident
    with depthwise_doubles.installed() as nat:
        net, info, x = _tiny(per_channel)
        for name in ("dw1", "dw2", "dw3"):
            assert all(1 <= s <= 16 for s in dn.shifts(info, name)), (name, dn.shifts(info, name))    # bits the kernel takes
        with torch.no_grad():
            plain = net(x)
        assert float(plain.abs().max()) > 0
        off = resident.enable(net, x, depthwise=False)
        off_plans = resident.describe(net)
        assert "resident_depthwise" not in off or off["resident_depthwise"] == 0
        for name in ("dw1", "dw2", "dw3"):
            assert name not in off_plans                                   # a grouped convolution stays a plain fp32 producer
        assert off_plans["stem"].emit_f32 and off_plans["pw1"].emit_f32      # ... and its producer has to write fp32 for it
        resident.disable(net)

        calls = []
        real = nat.dwconv2d_i8_resident
        nat.dwconv2d_i8_resident = lambda *a: (calls.append(a[5]), real(*a))[1]
        try:
            on = resident.enable(net, x, depthwise=True)                    # verify=True: bit-identical to the traced forward
            plans = resident.describe(net)
            assert on["resident_depthwise"] == 3 and on["resident_convs"] == off["resident_convs"] + 3, (on, off)
            assert on["fused_relus"] == off["fused_relus"] + 3, (on, off)  # r1, r3, r5
            for name in ("dw1", "dw2", "dw3"):
                p = plans[name]
                assert p.depthwise and p.emit_int and not p.emit_f32 and p.relu and not p.defer, (name, p)
            # their producers no longer write fp32, and no depthwise layer is run by an add or fused as a block tail
            assert not plans["stem"].emit_f32 and not plans["pw1"].emit_f32 and not plans["pw2"].emit_f32
            assert plans["pw3"].defer and not plans["pw3"].depthwise and plans["Eltwise"].fuse_next is None
            for relu in ("r1", "r3", "r5"):
                assert "forward" in getattr(net, relu).__dict__
            calls[:] = []
            with torch.no_grad():
                assert torch.equal(net(x), plain)
                assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
                assert torch.equal(net(x[:1]), plain[:1])
            assert len(calls) == 9                                          # three layers, three forwards
            if per_channel:
                assert all(isinstance(rs, nat.ShiftVec) for rs in calls)    # list bits go through the _pcs entry point
            else:
                assert all(isinstance(rs, int) for rs in calls)
            resident.disable(net)
            assert not resident.describe(net) and "forward" not in net.r1.__dict__
            calls[:] = []
            with torch.no_grad():
                assert torch.equal(net(x), plain)
            assert not calls                                                # the default forward again
        finally:
            nat.dwconv2d_i8_resident = real


def test_without_the_argument_the_plan_is_todays():
    from common.quantity import resident
    with depthwise_doubles.installed():
        for make in (_tiny, _add_net):
            net, _info, x = make()
            a = resident.enable(net, x)
            rows_default = _plan_rows(net)
            b = resident.enable(net, x, depthwise=False)
            rows_off = _plan_rows(net)
            assert a == b and rows_default == rows_off and rows_default
            assert not any(r[PLAN_FIELDS.index("depthwise")] for r in rows_default.values())
            assert set(a) == {"resident_convs", "resident_adds", "resident_pools", "fused_relus", "fp32_outputs", "int_only_outputs",
                              "fused_conv_adds", "fused_block_tails", "fused_projections"}          # the keys as they were
            resident.enable(net, x, depthwise=True)
            assert _plan_rows(net) != rows_default


def test_a_depthwise_output_feeds_an_add_as_a_resident_operand_and_the_plan_pickles():
    from common.quantity import resident
    with depthwise_doubles.installed():
        for per_channel in (False, "depthwise"):
            net, info, x = _add_net(per_channel)
            assert all(1 <= s <= 16 for n in ("dwa", "dwb") for s in dn.shifts(info, n))
            with torch.no_grad():
                plain = net(x)
            off = resident.enable(net, x)
            on = resident.enable(net, x, depthwise=True)
            plans = resident.describe(net)
            assert on["resident_depthwise"] == 2 and on["resident_convs"] == off["resident_convs"] + 2
            # dwa feeds the add directly: an integer operand, never deferred into it (the fused conv + add kernel is an MFMA kernel)
            assert plans["dwa"].depthwise and plans["dwa"].emit_int and not plans["dwa"].emit_f32 and not plans["dwa"].defer
            assert not plans["dwa"].relu and plans["Eltwise"].resident_add and plans["Eltwise"].fuse_arg is None
            assert plans["Eltwise"].relu and on["fused_conv_adds"] == 0
            assert plans["dwb"].depthwise and plans["dwb"].relu and not plans["dwb"].emit_f32       # reads the add's int8 form
            with torch.no_grad():
                assert torch.equal(net(x), plain)
                mid = net.dwa(net.r0(net.stem(x)))
            assert type(mid).__name__ == "QHandle" and mid.exact.dtype == torch.int8 and mid.exact.shape[-1] == 32
            assert not mid.exact[..., 19:].any()
            # derived weights are dropped from the pickle and rebuilt; the plan travels with the modules
            assert "_w_dw" in net.dwa.__dict__
            buf = io.BytesIO()
            pickle.dump(net, buf)
            again = pickle.loads(buf.getvalue())
            assert "_w_dw" not in again.dwa.__dict__ and resident.describe(again)["dwa"].depthwise
            with torch.no_grad():
                assert torch.equal(again(x), plain)
            resident.disable(net)
            with torch.no_grad():
                assert torch.equal(net(x), plain)


def test_the_instance_switch_runs_the_kernel_without_a_plan_and_gives_the_same_tensor():
    with depthwise_doubles.installed() as nat:
        from common.quantity import NewConv2d
        assert NewConv2d.use_depthwise_i8 is False
        for per_channel in (False, "depthwise"):
            net, _info, x = _tiny(per_channel)
            with torch.no_grad():
                h = net.r0(net.stem(x))
                want = net.dw2(net.r2(net.pw1(net.r1(net.dw1(h)))))
            calls = []
            real = nat.dwconv2d_i8_resident
            nat.dwconv2d_i8_resident = lambda *a: (calls.append(1), real(*a))[1]
            try:
                net.dw1.use_depthwise_i8 = True
                net.dw2.use_depthwise_i8 = True
                assert not net.dw1._int8_ok(net.dw1.Conv) and net.dw1._depthwise_ok(net.dw1.Conv)
                with torch.no_grad():
                    got = net.dw2(net.r2(net.pw1(net.r1(net.dw1(h)))))
            finally:
                nat.dwconv2d_i8_resident = real
            assert len(calls) == 2 and isinstance(got, torch.Tensor) and torch.equal(got, want)
            assert not net.dw3._depthwise_ok(net.dw3.Conv)                  # the class default stays off


def test_depthwise_ok_declines_what_the_kernel_does_not_take():
    from common.quantity import NewConv2d

    def layer(conv, ib=4, ob=4, wb=5):
        m = NewConv2d(conv, {"weight_bit": wb, "bias_bit": ob, "input_bit": ib, "output_bit": ob})
        m.use_depthwise_i8 = True
        return m

    ok = layer(nn.Conv2d(16, 16, 3, padding=1, groups=16))
    assert ok._depthwise_ok(ok.Conv) and ok._depthwise_ok(ok.Conv, True)
    ok.use_depthwise_i8 = False
    assert not ok._depthwise_ok(ok.Conv) and ok._depthwise_ok(ok.Conv, True)      # `True`: the switch taken as on (enable())
    m = layer(nn.Conv2d(20, 20, 5, stride=2, padding=4, groups=20))
    assert m._depthwise_ok(m.Conv)
    for name, conv, kw in [
            ("groups 4", nn.Conv2d(16, 16, 3, padding=1, groups=4), {}),
            ("multiplier 2", nn.Conv2d(16, 32, 3, padding=1, groups=16), {}),
            ("dense", nn.Conv2d(16, 16, 3, padding=1), {}),
            ("circular", nn.Conv2d(16, 16, 3, padding=1, groups=16, padding_mode="circular"), {}),
            ("string padding", nn.Conv2d(16, 16, 3, padding="same", groups=16), {}),
            ("dilation 2", nn.Conv2d(16, 16, 3, padding=2, dilation=2, groups=16), {}),
            ("7x7", nn.Conv2d(16, 16, 7, padding=3, groups=16), {}),
            ("1x1", nn.Conv2d(16, 16, 1, groups=16), {}),
            ("3x5", nn.Conv2d(16, 16, (3, 5), padding=1, groups=16), {}),
            ("stride 3", nn.Conv2d(16, 16, 3, stride=3, padding=1, groups=16), {}),
            ("stride 1x2", nn.Conv2d(16, 16, 3, stride=(1, 2), padding=1, groups=16), {}),
            ("padding 3", nn.Conv2d(16, 16, 3, padding=3, groups=16), {}),
            ("rs 0", nn.Conv2d(16, 16, 3, padding=1, groups=16), {"wb": 0, "ib": 4, "ob": 4}),
            ("rs 17", nn.Conv2d(16, 16, 3, padding=1, groups=16), {"wb": 12, "ib": 6, "ob": 1}),
            ("rs 0..5 per channel", nn.Conv2d(16, 16, 3, padding=1, groups=16), {"wb": [0] + [5] * 15}),
            ("rs 5..17 per channel", nn.Conv2d(16, 16, 3, padding=1, groups=16), {"wb": [17] + [5] * 15})]:
        m = layer(conv, **kw)
        assert not m._depthwise_ok(m.Conv), name
    for wb in (1, 16, [1] * 8 + [16] * 8):                                    # the ends of the shift range are taken
        m = layer(nn.Conv2d(16, 16, 3, padding=1, groups=16), wb=wb)
        assert m._depthwise_ok(m.Conv), wb
    assert not ok._depthwise_ok(nn.Linear(4, 4), True)


def test_kernel_address_arithmetic_stays_inside_its_tensors(tmp_path):
    """csrc/fq_dwconv_i8_geom.h holds the depthwise kernel's tile / lane -> address functions and compiles as host code:
    scripts/dwconv_geom_check.cpp walks every lane of every launch over the GPU tests' shapes and exits non-zero on a load
    outside the input, a store outside the output, or an output dword written twice or not at all."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "dwconv_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-o", exe, os.path.join(root, "scripts", "dwconv_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,"), out.stdout + out.stderr
