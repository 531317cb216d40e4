"""resident.enable(..., grouped=True) and NewConv2d.use_grouped_i8 on a box without a GPU: the tracer, the plan, the handles
and the module glue run for real; the kernel entry points are oracle-backed doubles (tests/native_doubles.py,
tests/depthwise_doubles.py, tests/grouped_doubles.py) that follow the reference's fp32 chain literally.  Every comparison is
exact."""
import io
import json
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

import cases
import grouped_doubles as gd
import grouped_nets as gn
from workdir_util import product_workdir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the fields of a plan as they were before this switch existed
PARENT_FIELDS = ("relu", "emit_f32", "emit_int", "narrow_bit", "want_wide", "grid", "resident_add", "defer", "fuse_arg",
                 "fuse_next", "narrow_to_hbm", "fuse_proj", "depthwise", "up")
PARENT_KEYS = {"resident_convs", "resident_adds", "resident_pools", "fused_relus", "fp32_outputs", "int_only_outputs",
               "fused_conv_adds", "fused_block_tails", "fused_projections"}
NETS = {"resnext": gn.ToyResNeXt, "pointwise": gn.GroupedPointwiseNet, "mixed": gn.GroupedDepthwiseNet, "add": gn.GroupedAddNet}


def _net(cls, per_channel=False, seed=3):
    model = gn.seeded(cls().eval(), seed=seed)
    info = gn.fixed_info(model, per_channel=per_channel)
    return gn.rebuild(model, info), info, torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))


def _rows(model, fields=PARENT_FIELDS):
    from common.quantity import resident
    return {name: tuple(getattr(p, f) for f in fields) for name, p in resident.describe(model).items()}


def _counting(nat):
    calls = []
    real = nat.gconv2d_i8_resident
    nat.gconv2d_i8_resident = lambda *a: (calls.append(a[7]), real(*a))[1]
    return calls, real


# ---------------------------------------------------------------- 1. the geometry walker and the header
def test_kernel_index_arithmetic_stays_inside_its_tensors_over_the_gpu_tests_shapes(tmp_path):
    """csrc/fq_gconv_i8_geom.h holds the grouped kernel's workgroup / lane -> tile, address, tap, LDS index and channel mask
    functions and compiles as host code: scripts/gconv_geom_check.cpp walks every lane of every launch over the GPU tests' shapes
    and the model's layers, and its shape list is the GPU tests' own (grouped_doubles.kernel_shapes)."""
    exe = str(tmp_path / "gconv_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "scripts", "gconv_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok,"), out.stdout + out.stderr
    listed = subprocess.run([exe, "--list"], capture_output=True, text=True)
    assert listed.returncode == 0
    assert [tuple(int(v) for v in ln.split()) for ln in listed.stdout.splitlines()] == gd.kernel_shapes()
    assert int(re.search(r"ok, (\d+) shapes", out.stdout).group(1)) == len(gd.kernel_shapes()) + 7       # + the model's layers


def test_host_emulation_of_the_kernels_loops_computes_the_grouped_convolution(tmp_path):
    """scripts/gconv_emul_check.cpp: the kernel's loops in C++ over the geometry header, against a direct grouped convolution."""
    exe = str(tmp_path / "gconv_emul_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "scripts", "gconv_emul_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok 576 cases"), out.stdout + out.stderr


def test_the_header_declares_the_entry_points_and_the_version_stays():
    from common.quantity import _native
    text = open(os.path.join(ROOT, "include", "fq.h")).read()
    for name in ("fq_gconv2d_i8_supported", "fq_gconv2d_i8_resident", "fq_gconv2d_i8_resident_pcs"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert hasattr(_native.lib(), name)
    assert re.search(r"#define\s+FQ_VERSION\s+103\b", text) and _native.lib().fq_version() == 103
    assert _native.CONV_VARIANTS[15] == "grouped" and _native.CONV_VARIANTS[14] == "depthwise"


# ---------------------------------------------------------------- 2. what the switch takes
def _layer(conv, ib=4, ob=4, wb=5):
    from common.quantity import NewConv2d
    m = NewConv2d(conv, {"weight_bit": wb, "bias_bit": ob, "input_bit": ib, "output_bit": ob})
    m.use_grouped_i8 = True
    return m


def _agrees(m):
    from common.quantity import _native
    c = m.Conv
    return _native.gconv_supported(c.in_channels, c.out_channels, c.groups, c.kernel_size[0], c.kernel_size[1], c.stride,
                                   c.dilation, m._rs())


def test_grouped_ok_takes_the_widths_and_geometries_of_the_kernel():
    from common.quantity import NewConv2d
    assert NewConv2d.use_grouped_i8 is False
    for (G, cgi, cgo) in gd.GROUP_WIDTHS:
        for k in (1, 3):
            for stride in (1, 2):
                for pad in range(k):
                    m = _layer(nn.Conv2d(G * cgi, G * cgo, k, stride=stride, padding=pad, groups=G))
                    assert m._grouped_ok(m.Conv) and _agrees(m), (G, cgi, cgo, k, stride, pad)
                    assert not m._int8_ok(m.Conv) and not m._depthwise_ok(m.Conv, True)
    ok = _layer(nn.Conv2d(32, 32, 3, padding=1, groups=8))
    ok.use_grouped_i8 = False                                                  # the switch is read per instance
    assert not ok._grouped_ok(ok.Conv) and ok._grouped_ok(ok.Conv, True)
    other = _layer(nn.Conv2d(32, 32, 3, padding=1, groups=8))
    assert other._grouped_ok(other.Conv) and not other._grouped_ok(other.Conv, False)
    for wb in (1, 16, [1] * 16 + [16] * 16):                                    # the ends of the shift range are taken
        m = _layer(nn.Conv2d(32, 32, 3, padding=1, groups=8), wb=wb)
        assert m._grouped_ok(m.Conv) and _agrees(m), wb
    assert not ok._grouped_ok(nn.Linear(4, 4), True)


def test_grouped_ok_declines_what_the_kernel_does_not_take():
    geometry = [                                                                # declined by the kernel's own rule as well
        ("dense", nn.Conv2d(32, 32, 3, padding=1), {}),
        ("depthwise", nn.Conv2d(32, 32, 3, padding=1, groups=32), {}),
        ("cgi 2", nn.Conv2d(32, 64, 3, padding=1, groups=16), {}),
        ("cgi 6", nn.Conv2d(24, 16, 3, padding=1, groups=4), {}),
        ("cgi 68", nn.Conv2d(136, 16, 3, padding=1, groups=2), {}),
        ("cgo 3", nn.Conv2d(32, 24, 3, padding=1, groups=8), {}),
        ("5x5", nn.Conv2d(32, 32, 5, padding=2, groups=8), {}),
        ("3x1", nn.Conv2d(32, 32, (3, 1), padding=(1, 0), groups=8), {}),
        ("dilation 2", nn.Conv2d(32, 32, 3, padding=2, dilation=2, groups=8), {}),
        ("stride 3", nn.Conv2d(32, 32, 3, stride=3, padding=1, groups=8), {}),
        ("stride 1x2", nn.Conv2d(32, 32, 3, stride=(1, 2), padding=1, groups=8), {}),
        ("rs 0", nn.Conv2d(32, 32, 3, padding=1, groups=8), {"wb": 0, "ib": 4, "ob": 4}),
        ("rs 17", nn.Conv2d(32, 32, 3, padding=1, groups=8), {"wb": 12, "ib": 6, "ob": 1}),
        ("rs 0..5 per channel", nn.Conv2d(32, 32, 3, padding=1, groups=8), {"wb": [0] + [5] * 31}),
        ("rs 5..17 per channel", nn.Conv2d(32, 32, 3, padding=1, groups=8), {"wb": [17] + [5] * 31})]
    for name, conv, kw in geometry:
        m = _layer(conv, **kw)
        assert not m._grouped_ok(m.Conv) and not m._grouped_ok(m.Conv, True) and not _agrees(m), name
    module = [                                                                  # declined before the kernel's rule is asked
        ("padding 3", nn.Conv2d(32, 32, 3, padding=3, groups=8)),
        ("padding 1 of a 1x1", nn.Conv2d(32, 32, 1, padding=1, groups=8)),
        ("padding (0, 3)", nn.Conv2d(32, 32, 3, padding=(0, 3), groups=8)),
        ("string padding", nn.Conv2d(32, 32, 3, padding="same", groups=8)),
        ("circular", nn.Conv2d(32, 32, 3, padding=1, groups=8, padding_mode="circular"))]
    for name, conv in module:
        m = _layer(conv)
        assert not m._grouped_ok(m.Conv) and not m._grouped_ok(m.Conv, True), name


# ---------------------------------------------------------------- 3. plans of the toy nets
@pytest.mark.parametrize("per_channel", [False, "grouped"], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("tag", ["resnext", "pointwise"])
def test_grouped_layers_become_integer_layers(tag, per_channel):
    from common.quantity import resident
    cls = NETS[tag]
    with gd.installed() as nat:
        net, info, x = _net(cls, per_channel)
        for name in cls.GROUPED:
            assert all(1 <= s <= 16 for s in gn.shifts(info, name)), (name, gn.shifts(info, name))    # bits the kernel takes
        with torch.no_grad():
            plain = net(x)
        assert float(plain.abs().max()) > 0
        off = resident.enable(net, x)
        off_plans = resident.describe(net)
        assert set(off) == PARENT_KEYS
        front = {"resnext": ("b1.conv1", "b2.conv1"), "pointwise": ("stem", "mid")}[tag]
        for name in cls.GROUPED:
            assert name not in off_plans                                   # a grouped convolution stays a plain fp32 producer
        for name in front:
            assert off_plans[name].emit_f32                                # ... and the layer in front has to write fp32 for it
        resident.disable(net)

        calls, real = _counting(nat)
        try:
            on = resident.enable(net, x, grouped=True)                      # verify=True: bit-identical to the traced forward
            plans = resident.describe(net)
            n = len(cls.GROUPED)
            assert on["resident_grouped"] == n and on["resident_convs"] == off["resident_convs"] + n, (on, off)
            assert on["fused_relus"] == off["fused_relus"] + n, (on, off)
            assert on["fused_conv_adds"] >= off["fused_conv_adds"] and on["fused_block_tails"] >= off["fused_block_tails"]
            assert on["fused_projections"] >= off["fused_projections"] and on["fp32_outputs"] == off["fp32_outputs"] - n
            for name in cls.GROUPED:
                p = plans[name]
                assert p.grouped and p.emit_int and not p.emit_f32 and p.relu and not p.defer and not p.depthwise, (name, p)
            for name in front:                                             # from emit_f32 to integer-only
                assert not plans[name].emit_f32 and plans[name].emit_int and not plans[name].grouped
            for name, p in plans.items():                                  # no grouped layer is run by an add or as a block tail
                assert p.fuse_next is None or not plans[[k for k, m in net.named_modules() if m is p.fuse_next][0]].grouped
            if tag == "resnext":
                assert plans["b1.conv3"].defer and plans["b2.conv3"].defer and not plans["b1.conv3"].grouped
            calls[:] = []
            with torch.no_grad():
                assert torch.equal(net(x), plain)
                assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
                assert torch.equal(net(x[:1]), plain[:1])
            assert len(calls) == 3 * n                                      # every grouped layer, three forwards
            if per_channel:
                assert all(isinstance(rs, nat.ShiftVec) for rs in calls)    # list bits go through the _pcs entry point
            else:
                assert all(isinstance(rs, int) for rs in calls)
            resident.disable(net)
            assert not resident.describe(net)
            calls[:] = []
            with torch.no_grad():
                assert torch.equal(net(x), plain)
            assert not calls                                                # the default forward again
        finally:
            nat.gconv2d_i8_resident = real


def test_without_the_argument_the_plan_is_todays():
    from common.quantity import resident
    with gd.installed():
        for cls in NETS.values():
            net, _info, x = _net(cls)
            a = resident.enable(net, x)
            rows_default = _rows(net)
            b = resident.enable(net, x, grouped=False)
            rows_off = _rows(net)
            assert a == b and rows_default == rows_off and rows_default
            assert set(a) == PARENT_KEYS and "resident_grouped" not in a                          # the keys as they were
            assert not any(p.grouped for p in resident.describe(net).values())
            for name in cls.GROUPED:
                assert name not in rows_default
            on = resident.enable(net, x, grouped=True)
            assert set(on) == PARENT_KEYS | {"resident_grouped"} and _rows(net) != rows_default


def test_depthwise_and_grouped_combine():
    from common.quantity import resident
    with gd.installed():
        for per_channel in (False, "grouped"):
            net, info, x = _net(gn.GroupedDepthwiseNet, per_channel)
            assert all(1 <= s <= 16 for n in ("gc", "dw") for s in gn.shifts(info, n))
            with torch.no_grad():
                plain = net(x)
            only_dw = resident.enable(net, x, depthwise=True)
            assert only_dw["resident_depthwise"] == 1 and "resident_grouped" not in only_dw and "gc" not in resident.describe(net)
            only_gc = resident.enable(net, x, grouped=True)
            assert only_gc["resident_grouped"] == 1 and "resident_depthwise" not in only_gc and "dw" not in resident.describe(net)
            both = resident.enable(net, x, depthwise=True, grouped=True)
            plans = resident.describe(net)
            assert both["resident_grouped"] == 1 and both["resident_depthwise"] == 1 and both["fp32_outputs"] == 0
            assert plans["gc"].grouped and not plans["gc"].depthwise and plans["dw"].depthwise and not plans["dw"].grouped
            assert not plans["gc"].emit_f32 and not plans["dw"].emit_f32 and not plans["stem"].emit_f32
            with torch.no_grad():
                assert torch.equal(net(x), plain) and torch.equal(net(x[:1]), plain[:1])


def test_a_grouped_output_feeds_an_add_as_a_resident_operand_and_the_plan_pickles():
    from common.quantity import resident
    with gd.installed():
        for per_channel in (False, "grouped"):
            net, info, x = _net(gn.GroupedAddNet, per_channel)
            assert all(1 <= s <= 16 for n in ("ga", "gb") for s in gn.shifts(info, n))
            with torch.no_grad():
                plain = net(x)
            off = resident.enable(net, x)
            on = resident.enable(net, x, grouped=True)
            plans = resident.describe(net)
            assert on["resident_grouped"] == 2 and on["resident_convs"] == off["resident_convs"] + 2
            # ga feeds the add directly: an integer operand, never deferred into it (the fused conv + add kernel is an MFMA kernel)
            assert plans["ga"].grouped and plans["ga"].emit_int and not plans["ga"].emit_f32 and not plans["ga"].defer
            assert not plans["ga"].relu and plans["Eltwise"].resident_add and plans["Eltwise"].fuse_arg is None
            assert plans["Eltwise"].relu and on["fused_conv_adds"] == 0
            assert plans["gb"].grouped and plans["gb"].relu and not plans["gb"].emit_f32           # reads the add's int8 form
            with torch.no_grad():
                assert torch.equal(net(x), plain)
                mid = net.ga(net.r0(net.stem(x)))
            assert type(mid).__name__ == "QHandle" and mid.exact.dtype == torch.int8 and mid.exact.shape[-1] == 32
            assert not mid.exact[..., 24:].any()
            # derived weights are dropped from the pickle and rebuilt; the plan travels with the modules
            assert "_w_gc" in net.ga.__dict__
            buf = io.BytesIO()
            pickle.dump(net, buf)
            again = pickle.loads(buf.getvalue())
            assert "_w_gc" not in again.ga.__dict__ and resident.describe(again)["ga"].grouped
            with torch.no_grad():
                assert torch.equal(again(x), plain)
            resident.disable(net)
            with torch.no_grad():
                assert torch.equal(net(x), plain)


def test_a_plan_pickled_before_the_switch_existed_still_loads():
    from common.quantity import resident
    p = resident.Plan()
    old = {k: v for k, v in p.__getstate__().items() if k != "grouped"}
    q = resident.Plan.__new__(resident.Plan)
    q.__setstate__(old)
    assert q.grouped is False and q.__getstate__() == p.__getstate__()


def test_a_grouped_layer_called_twice_is_not_planned():
    from common.quantity import resident
    with gd.installed() as nat:
        net, _info, x = _net(gn.TwiceNet)
        assert net.gc._grouped_ok(net.gc.Conv, True)
        with torch.no_grad():
            plain = net(x)
        calls, real = _counting(nat)
        try:
            on = resident.enable(net, x, grouped=True)
            assert on["resident_grouped"] == 0 and "gc" not in resident.describe(net)
            with torch.no_grad():
                assert torch.equal(net(x), plain)
            assert not calls
        finally:
            nat.gconv2d_i8_resident = real


def test_the_instance_switch_runs_the_kernel_without_a_plan_and_gives_the_same_tensor():
    with gd.installed() as nat:
        for per_channel in (False, "grouped"):
            net, _info, x = _net(gn.ToyResNeXt, per_channel)
            with torch.no_grad():
                h = net.b1.relu1(net.b1.conv1(net.r0(net.stem(x))))
                want = net.b1.conv2(h)
            calls, real = _counting(nat)
            try:
                net.b1.conv2.use_grouped_i8 = True
                assert not net.b1.conv2._int8_ok(net.b1.conv2.Conv) and net.b1.conv2._grouped_ok(net.b1.conv2.Conv)
                with torch.no_grad():
                    got = net.b1.conv2(h)
            finally:
                nat.gconv2d_i8_resident = real
            assert len(calls) == 1 and isinstance(got, torch.Tensor) and got.dtype == torch.float32 and torch.equal(got, want)
            assert not net.b2.conv2._grouped_ok(net.b2.conv2.Conv)         # the class default stays off


# ---------------------------------------------------------------- 4. golden G16: a calibrated ResNeXt-style net
@pytest.fixture(scope="module")
def g16(golden_dir):
    with open(os.path.join(golden_dir, "g16_grouped_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g16_grouped_net.npz"))


def test_g16_cpu_engine_matches_the_reference_with_the_switch_on_and_off(g16, oracle):
    """The reference's graph discovery, merge groups, feat.table and weight.table of grouped_nets.g16_net byte for byte through
    the oracle-backed CPU engine, and its ReconModel logits bit for bit: plain, with the parent's plan and with grouped=True."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    ref, arrays = g16
    shape = gn.G16_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(cases.seed_model(gn.g16_net(), base_seed=gn.G16_SEED).eval())
        got = {"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "cared_op_layer_names": q.cared_op_layer_names,
               "merge_groups": q.get_merge_groups(q.net_info), "layers_num": q.layers_num}
        q.activation_quantize(cases.calib_batches(3, shape, seed=gn.G16_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        got["feat_table"] = open(os.path.join(wd, "feat.table")).read()
        q.weight_quantize()
        got["weight_table"] = open(os.path.join(wd, "weight.table")).read()
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table"):
            assert got[key] == ref[key], key
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(cases.seed_model(gn.g16_net(), base_seed=gn.G16_SEED).eval())
        info = rec.get_quantity_information()
        assert sorted(info.keys()) == ref["recon_layers"]
        with gd.installed():
            net = rec.ReconModel(info, os.path.join(wd, "recon.pth"))
            x = cases.fixed_input(shape, seed=gn.G16_INPUT_SEED)
            np.testing.assert_array_equal(x.numpy(), arrays["x"])
            taken = [n for n in gn.ToyResNeXt.GROUPED if getattr(net, n.split(".")[0]).conv2._grouped_ok(getattr(net, n.split(".")[0]).conv2.Conv, True)]
            assert taken == list(gn.ToyResNeXt.GROUPED)                     # the calibrated shifts are ones the kernel takes
            with torch.no_grad():
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                off = resident.enable(net, x)
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                on = resident.enable(net, x, grouped=True)
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                np.testing.assert_array_equal(net(x[:1]).numpy(), arrays["logits_recon"][:1])
            assert on["resident_grouped"] == 2 and on["resident_convs"] == off["resident_convs"] + 2, (off, on)
            assert "resident_grouped" not in off
