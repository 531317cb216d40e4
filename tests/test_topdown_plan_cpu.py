"""resident.enable(..., concat=True, topdown=True) on a box without a GPU: a NewAdd reads one operand through a nearest upsampling
-- the FPN top-down step -- over an int8 activation or the exact int16 sum of the add one level up.  The tracer, the plan, the
handles and the module glue run for real; the kernel entry points are oracle-backed doubles (tests/topdown_doubles.py on top of
every other double) that follow the reference's fp32 chain literally.  Every comparison is exact.  The kernel's address arithmetic
is walked on the host (scripts/add_up_geom_check.cpp), golden G24 pins a calibrated toy FPN to the reference, and forty random
FPN-shaped nets run under three plans."""
import io
import json
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

import cases
import mixed_nets as mn
import topdown_doubles
import topdown_nets as tn
from workdir_util import product_workdir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_TEN = dict(depthwise=True, concat=True, avgpool=True, grouped=True, relu6=True, flatten=True, shuffle=True, activations=True,
               sums=True, topdown=True)
SLOTS = ("relu", "emit_f32", "emit_int", "narrow_bit", "want_wide", "grid", "resident_add", "defer", "fuse_arg", "fuse_next",
         "narrow_to_hbm", "fuse_proj", "depthwise", "up", "grouped", "clip", "perm", "table")


def _plans(model):
    from common.quantity import resident
    return resident.describe(model)


def _rows(model):
    return {n: tuple(getattr(p, f) for f in p.__slots__) for n, p in _plans(model).items()}


def _tuple(t):
    return t if isinstance(t, tuple) else (t,)


def _same(a, b):
    a, b = _tuple(a), _tuple(b)
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def _check_forwards(net, x, plain):
    """the example, one image, a flipped batch"""
    with torch.no_grad():
        assert _same(net(x), plain)
        assert _same(net(x[:1]), tuple(p[:1] for p in _tuple(plain)))
        assert _same(net(torch.flip(x, dims=[0])), tuple(torch.flip(p, dims=[0]) for p in _tuple(plain)))


class _Spy(object):
    """Records the calls of add_up_resident, add_resident and the stand-alone upsampling launch while installed."""

    def __init__(self, nat):
        self.nat, self.up, self.flat, self.moved = nat, [], [], []

    def __enter__(self):
        self.real = (self.nat.add_up_resident, self.nat.add_resident, self.nat.concat_i8_nhwc)
        self.nat.add_up_resident = lambda *a, **k: (self.up.append((a[0].dtype, a[2].dtype) + tuple(a[4:])), self.real[0](*a, **k))[1]
        self.nat.add_resident = lambda *a, **k: (self.flat.append((a[0].dtype, a[2].dtype)), self.real[1](*a, **k))[1]
        self.nat.concat_i8_nhwc = lambda *a, **k: (self.moved.append(len(a[0])), self.real[2](*a, **k))[1]
        return self

    def __exit__(self, *exc):
        self.nat.add_up_resident, self.nat.add_resident, self.nat.concat_i8_nhwc = self.real

    def clear(self):
        self.up[:], self.flat[:], self.moved[:] = [], [], []


# ---------------------------------------------------------------- 1. the switch and the entry points
def test_topdown_needs_concat():
    from common.quantity import resident
    with topdown_doubles.installed():
        net = tn.TopDownNet().eval()
        for kw in (dict(topdown=True), dict(topdown=True, concat=False), dict(topdown=True, avgpool=True, sums=True)):
            with pytest.raises(ValueError, match="concat=True"):
                resident.enable(net, net.example(), **kw)
        assert not resident.is_enabled(net)


def test_the_binding_and_the_header_symbol_exist():
    from common.quantity import _native
    assert callable(_native.add_up_resident) and callable(_native.add_up_supported)
    with open(os.path.join(ROOT, "include", "fq.h")) as fh:
        text = fh.read()
    assert "int fq_add_up_resident(" in text and "int fq_add_up_resident_supported(int up, int H, int W, int Cpad);" in text


def test_add_up_supported_is_host_arithmetic():
    from common.quantity import _native
    ok = _native.add_up_supported
    assert ok(2, 2, 2, 16) and ok(4, 4, 12, 112) and ok(2, 56, 56, 256) and ok(4, 8, 8, 16)
    assert not ok(3, 6, 6, 16) and not ok(1, 4, 4, 16) and not ok(8, 8, 8, 16) and not ok(0, 4, 4, 16)
    assert not ok(2, 3, 4, 16) and not ok(2, 4, 3, 16) and not ok(4, 6, 8, 16) and not ok(4, 2, 2, 16)
    assert not ok(2, 4, 4, 8) and not ok(2, 4, 4, 0) and not ok(2, 0, 4, 16) and not ok(2, 4, -2, 16)


def test_the_double_is_the_add_double_on_the_repeated_operand():
    with topdown_doubles.installed() as nat:
        rng = np.random.default_rng(24)
        for (xd, yd, gx, gy, up) in ((np.int8, np.int8, 4, 3, 2), (np.int8, np.int16, 2, 5, 4), (np.int16, np.int8, 6, 4, 2),
                                     (np.int16, np.int16, 3, 3, 4)):
            x = tn.source(rng, (2, 8, 8, 32), 19, xd, gx)
            y = tn.source(rng, (2, 8 // up, 8 // up, 32), 19, yd, gy)
            g = max(0, gx, gy)
            wide, narrow = nat.add_up_resident(torch.from_numpy(x), gx, torch.from_numpy(y), gy, up, True, g, True, 4, True)
            w2, n2 = nat.add_resident(torch.from_numpy(x), gx, torch.from_numpy(tn.repeat(y, up)), gy, True, g, True, 4, True)
            assert torch.equal(wide, w2) and torch.equal(narrow, n2) and wide.dtype == torch.int16 and narrow.dtype == torch.int8
            assert tuple(wide.shape) == x.shape


# ---------------------------------------------------------------- 2. what is planned
PLANNED = {
    "plain": dict(),
    "relu_behind_the_sums": dict(relu_sum=True),
    "upsampled_operand_first": dict(swap=True),
    "factor_4": dict(factor=4),
    "upsample_module": dict(up=lambda step: nn.Upsample(scale_factor=2.0, mode="nearest")),
    "operands_on_three_grids": dict(bits=(3, 5, 6), read_bits=(2, 6)),
    "grid_8_and_negative_bits": dict(bits=(-1, 8, 2), read_bits=(0, 7)),
}


@pytest.mark.parametrize("tag", sorted(PLANNED))
def test_the_two_step_pathway(tag):
    """Off: the first upsampling launches on int8 and add1 reads the large tensor; add1 writes fp32 for the second upsampling,
    torch runs it and add2 falls to add_sat.  On: both adds run on add_up_resident, the sums write integers only."""
    from common.quantity import resident
    with topdown_doubles.installed() as nat, _Spy(nat) as spy:
        net = tn.TopDownNet(**PLANNED[tag]).eval()
        x = net.example()
        with torch.no_grad():
            plain = net(x)
        assert all(float(p.abs().max()) > 0 for p in plain)
        off = resident.enable(net, x, concat=True)
        plans = _plans(net)
        assert "topdown_adds" not in off and not plans.topdown_left and "topdown_left" not in net.__dict__.get("_fq_resident_report", {})
        assert plans["add1"].emit_f32 and plans["add1"].resident_add and "up2" not in plans and "add2" not in plans
        assert plans["up1"].up == net.factor and not plans["up1"].defer
        spy.clear()
        _check_forwards(net, x, plain)
        assert not spy.up and len(spy.flat) == 3 and spy.moved == [1, 1, 1]

        on = resident.enable(net, x, concat=True, topdown=True)                # verify=True
        plans = _plans(net)
        assert set(on) == set(off) | {"topdown_adds", "topdown_sum_sources"} and not plans.topdown_left
        assert on["topdown_adds"] == 2 and on["topdown_sum_sources"] == 1
        assert on["fp32_outputs"] == off["fp32_outputs"] - 2 == 3               # the three output convolutions, which the model returns
        assert on["resident_adds"] == 2 and on["resident_upsamples"] == 2 and on["fused_conv_adds"] == 0
        a1, a2, u1, u2 = plans["add1"], plans["add2"], plans["up1"], plans["up2"]
        g1 = max(0, net.l4.output_bit, net.l3.output_bit)
        assert not a1.emit_f32 and a1.emit_int and a1.want_wide and a1.narrow_bit == net.o3.input_bit and a1.grid == g1
        assert not a2.emit_f32 and a2.resident_add and a2.narrow_bit == net.o2.input_bit and a2.grid == max(g1, net.l2.output_bit)
        assert a1.relu == a2.relu == net.relu_sum and a1.fuse_arg is None and a2.fuse_arg is None
        for u, g in ((u1, net.l4.output_bit), (u2, g1)):
            assert u.up == net.factor and u.defer and u.emit_int and not u.emit_f32 and not u.relu and u.narrow_bit == g
        for name in ("l4", "l3", "l2"):                                         # the laterals launch themselves
            assert not plans[name].defer and not plans[name].emit_f32
        assert isinstance(net.up2.__dict__["forward"], resident._UpsampleTopDown)
        spy.clear()
        _check_forwards(net, x, plain)
        assert len(spy.up) == 6 and not spy.flat and not spy.moved
        ib1, ib2 = net.o3.input_bit, net.o2.input_bit
        assert spy.up[0] == (torch.int8, torch.int8, net.factor, True, g1, True, ib1, net.relu_sum)
        assert spy.up[1] == (torch.int8, torch.int16, net.factor, False, a2.grid, True, ib2, net.relu_sum)
        # the handles: the sum in front carries wide and narrow, the upsampling hands on the coarse handle itself
        with torch.no_grad():
            c2 = net.r0(net.stem(x))
            c3 = net.r1(net.d1(c2))
            u = net.up1(net.l4(net.r2(net.d2(c3))))
            s3 = net.add1(u, net.l3(c3)) if net.swap else net.add1(net.l3(c3), u)
            if net.relu_sum:
                s3 = net.ra1(s3)
            u2h = net.up2(s3)
        assert type(u) is resident.DeferredUpsample and u.s == net.factor and u.handle.exact.dtype == torch.int8 and u._out is None
        assert type(s3) is resident.QHandle and s3.exact.dtype == torch.int16 and s3.narrow.dtype == torch.int8 and s3.grid == g1
        assert type(u2h) is resident.DeferredUpsample and u2h.handle is s3 and u2h._out is None and u2h.module is net.up2
        resident.disable(net)
        assert not _plans(net) and not _plans(net).topdown_left and all("forward" not in m.__dict__ for m in net.modules())
        assert not any(k.startswith("_fq_resident") for k in net.__dict__)
        spy.clear()
        _check_forwards(net, x, plain)
        assert not spy.up


DECLINED = {
    # tag: (net arguments, {upsampling: piece of its reason}, topdown_adds, topdown_sum_sources)
    "relu_behind_the_upsampling": (dict(mode="relu_behind"), {"up2": "a ReLU sits between"}, 1, 0),
    "module_called_twice": (dict(mode="twice"), {"up1": "called more than once"}, 0, 0),
    "second_reader_over_a_sum": (dict(mode="extra_reader"), {"up2": "read by side besides the NewAdd"}, 1, 0),
    "second_reader_over_int8": (dict(mode="extra_reader_int8"), {"up1": "read by side besides the NewAdd"}, 1, 1),
    "both_operands_upsampled": (dict(mode="both_up"), {"up1": "both operands", "up1b": "both operands"}, 1, 1),
    "other_operand_is_fp32": (dict(mode="foreign_lateral"), {"up2": "is not resident"}, 1, 0),
    "size_form": (dict(up=lambda step: nn.Upsample(size=(8 * step, 8 * step))), {"up1": "`size=` form", "up2": "`size=` form"}, 0, 0),
    "bilinear": (dict(up=lambda step: nn.Upsample(scale_factor=2, mode="bilinear")), {"up1": "another mode", "up2": "another mode"}, 0, 0),
}


@pytest.mark.parametrize("tag", sorted(k for k, v in DECLINED.items() if v[1] is not None))
def test_what_the_plan_declines_keeps_its_earlier_plan_and_says_why(tag):
    """Each declined upsampling is named in describe().topdown_left and its plan row -- and the rows of its source and of its
    readers -- are the ones enable(concat=True) alone gives; the other step of the pathway is still planned where the rule admits
    it."""
    from common.quantity import resident
    kw, reasons, n_adds, n_sums = DECLINED[tag]
    with topdown_doubles.installed() as nat, _Spy(nat) as spy:
        net = tn.TopDownNet(**kw).eval()
        x = net.example()
        with torch.no_grad():
            plain = net(x)
        off = resident.enable(net, x, concat=True)
        rows = _rows(net)
        on = resident.enable(net, x, concat=True, topdown=True)
        plans, rows_on = _plans(net), _rows(net)
        assert set(plans.topdown_left) == set(reasons), plans.topdown_left
        for name, why in reasons.items():
            assert why in plans.topdown_left[name], plans.topdown_left
            assert rows_on.get(name) == rows.get(name), (name, rows_on.get(name), rows.get(name))
            assert not isinstance(net.get_submodule(name).__dict__.get("forward"), resident._UpsampleTopDown)
        assert on["topdown_adds"] == n_adds and on["topdown_sum_sources"] == n_sums, on
        if n_adds == 0:
            assert rows_on == rows and {k: v for k, v in on.items() if not k.startswith("topdown_")} == off
        spy.clear()
        _check_forwards(net, x, plain)
        assert len(spy.up) == 3 * n_adds


def test_the_default_call_has_no_new_key_and_plan_slots_are_unchanged():
    from common.quantity import resident
    import concat_nets as cn
    with topdown_doubles.installed():
        net = tn.TopDownNet().eval()
        x = net.example()
        a = resident.enable(net, x)
        rows = _rows(net)
        assert set(a) == cn.DEFAULT_KEYS
        assert resident.enable(net, x, topdown=False) == a and rows == _rows(net)
        b = resident.enable(net, x, concat=True)
        rows_b = _rows(net)
        assert resident.enable(net, x, concat=True, topdown=False) == b and rows_b == _rows(net)
        assert not any(k.startswith("topdown") for k in list(a) + list(b)) and not _plans(net).topdown_left
        assert "topdown_left" not in net.__dict__.get("_fq_resident_report", {})
        assert set(next(iter(_plans(net).values())).__slots__) == set(SLOTS)
    assert resident.Plan.__slots__ == SLOTS


def test_a_planned_model_pickles_with_its_plan_and_disable_removes_it():
    from common.quantity import resident
    with topdown_doubles.installed():
        for kw in (dict(), dict(relu_sum=True, swap=True), dict(mode="extra_reader")):
            net = tn.TopDownNet(**kw).eval()
            x = net.example()
            with torch.no_grad():
                plain = net(x)
            resident.enable(net, x, concat=True, topdown=True)
            buf = io.BytesIO()
            pickle.dump(net, buf)
            again = pickle.loads(buf.getvalue())
            assert _rows(again) == _rows(net) and resident.is_enabled(again)
            assert isinstance(again.up1.__dict__["forward"], resident._UpsampleTopDown)
            assert _plans(again).topdown_left == _plans(net).topdown_left
            with torch.no_grad():
                assert _same(again(x), plain)
            resident.disable(again)
            assert not _plans(again) and "forward" not in again.up1.__dict__
            assert not any(k.startswith("_fq_resident") for k in again.__dict__)
            with torch.no_grad():
                assert _same(again(x), plain)


def test_run_time_misses_fall_back_to_values():
    """An add that is handed a deferred upsampling it cannot take goes on with the values: the int8 payload through the
    stand-alone upsampling launch, the int16 payload through the module's own forward on the de-quantised coarse tensor."""
    from common.quantity import resident
    with topdown_doubles.installed() as nat, _Spy(nat) as spy:
        net = tn.TopDownNet().eval()
        x = net.example()
        resident.enable(net, x, concat=True, topdown=True)
        spy.clear()                                                             # (enable's own verifying forward)
        with torch.no_grad():
            c2 = net.r0(net.stem(x))
            c3 = net.r1(net.d1(c2))
            lat3, lat2, p4 = net.l3(c3), net.l2(c2), net.l4(net.r2(net.d2(c3)))
            s3 = net.add1(lat3, net.up1(p4))
            want3, want2 = s3.to_f32(), net.o2(net.add2(lat2, net.up2(s3)))     # (add2 hands out its int8 form only: held through o2)
            assert len(spy.up) == 2 and not spy.flat and not spy.moved

            # int8 payload, the plan's grid disagrees: the upsampling is launched, the flat add reads its handle
            spy.clear()
            plan = net.add1.__dict__["_resident"]
            plan.grid += 1
            out = net.add1(lat3, net.up1(p4))
            plan.grid -= 1
            assert not spy.up and not spy.flat and spy.moved == [1] and torch.equal(as_tensor(out), want3)
            # int8 payload, a non-resident add: values
            spy.clear()
            plan.resident_add = False
            out = net.add1(lat3, net.up1(p4))
            plan.resident_add = True
            assert not spy.up and not spy.flat and spy.moved == [1] and torch.equal(as_tensor(out), want3)
            # int8 payload, materialised by somebody else first: the flat add on the materialised handle
            spy.clear()
            d = net.up1(p4)
            h = d.materialise()
            assert type(h) is resident.QHandle and h.exact.shape[1] == 2 * p4.exact.shape[1] and spy.moved == [1]
            out = net.add1(lat3, d)
            assert not spy.up and len(spy.flat) == 1 and torch.equal(out.to_f32(), want3)

            # int16 payload
            for miss in ("grid", "non_resident", "lossy", "materialised"):
                spy.clear()
                plan = net.add2.__dict__["_resident"]
                d = net.up2(s3)
                assert type(d) is resident.DeferredUpsample and d.handle.exact.dtype == torch.int16
                if miss == "grid":
                    plan.grid += 1
                elif miss == "non_resident":
                    plan.resident_add = False
                elif miss == "materialised":
                    f = d.materialise()
                    assert isinstance(f, torch.Tensor) and f.dtype == torch.float32 and torch.equal(f, nn.functional.interpolate(want3, scale_factor=2))
                    assert resident.resident_of(d) is None and d.to_f32() is f
                lossy = resident.QHandle(lat2.shape, lat2.exact, lat2.grid, lat2.narrow, lat2.bit, lat2.relu_done)
                lossy.lossy = miss == "lossy"
                try:
                    if miss == "lossy":
                        with pytest.raises(nat.FqError):                        # a table activation's integers are no summand
                            net.add2(lossy, d)
                        continue
                    out = net.add2(lat2, d)
                finally:
                    plan.grid, plan.resident_add = max(0, s3.grid, lat2.grid), True
                assert not spy.up and not spy.flat and not spy.moved and isinstance(out, torch.Tensor), miss
                assert torch.equal(net.o2(out), want2), miss
            # and the planned path again
            spy.clear()
            assert torch.equal(net.o2(net.add2(lat2, net.up2(s3))), want2) and len(spy.up) == 1
            # an upsampling that meets an input it was not planned for runs torch's forward
            f3 = s3.to_f32()
            assert torch.equal(net.up2(f3), nn.functional.interpolate(f3, scale_factor=2))
            other = resident.QHandle(s3.shape, s3.exact, s3.grid + 1, s3.narrow, s3.bit, s3.relu_done)
            assert torch.equal(net.up2(other), nn.functional.interpolate(other.to_f32(), scale_factor=2))


def as_tensor(out):
    return out.to_f32() if not isinstance(out, torch.Tensor) else out


# ---------------------------------------------------------------- 3. the walker
def test_kernel_address_arithmetic_stays_inside_its_tensors(tmp_path):
    """csrc/fq_add_up_geom.h holds the kernel's lane -> (item, offsets) functions and compiles as host code:
    scripts/add_up_geom_check.cpp walks every lane of every launch and exits non-zero on a load outside either source, an
    unaligned access, a coarse pixel that is not (h / up, w / up) or an output element written zero times or twice -- over its
    built-in list (the model's launch shapes among them) and over the GPU tests' shape list."""
    exe = str(tmp_path / "add_up_geom_check")
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "scripts", "add_up_geom_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1].startswith("ok,"), out.stdout + out.stderr
    shapes = tn.KERNEL_CASES + [tn.SECOND_ITEM_CASE]
    out = subprocess.run([exe] + [tn.case_arg(c) for c in shapes], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1].startswith("ok,") and len(lines) == len(shapes) + 1, out.stdout + out.stderr
    words = [ln for ln in lines if ln.startswith("case " + tn.case_arg(tn.SECOND_ITEM_CASE))][0].split()
    n, h, w, c, up = tn.SECOND_ITEM_CASE
    items = n * h * w * tn.pad16(c) // 16
    assert int(words[words.index("items") + 1]) == items > tn.LANES and int(words[words.index("blocks") + 1]) == 4096
    assert int(words[words.index("second-items") + 1]) == items - tn.LANES
    # the smallest square plane of this width: one coarse row and column less gives every lane at most one item
    assert n * (h - up) * (w - up) * tn.pad16(c) // 16 <= tn.LANES
    for bad in ("1,3,4,16,2", "1,4,4,16,3", "1,6,8,16,4"):
        assert subprocess.run([exe, bad], capture_output=True, text=True).returncode == 1


# ---------------------------------------------------------------- 4. golden G24: a calibrated toy FPN
@pytest.fixture(scope="module")
def g24(golden_dir):
    with open(os.path.join(golden_dir, "g24_topdown_net.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g24_topdown_net.npz"))


def test_g24_cpu_engine_matches_the_reference_with_the_switch_on_and_off(g24, oracle):
    """The reference's graph discovery, merge groups, feat.table, weight.table and quantity information of topdown_nets.g24_net
    byte for byte through the oracle-backed CPU engine, and its ReconModel logits bit for bit: plain, with concat=True and with
    concat=True, topdown=True."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    ref, arrays = g24
    shape = tn.G24_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(cases.seed_model(tn.g24_net(), base_seed=tn.G24_SEED).eval())
        got = {"net_info": dict(q.net_info), "net_info_order": list(q.net_info.keys()), "cared_op_layer_names": q.cared_op_layer_names,
               "merge_groups": q.get_merge_groups(q.net_info), "layers_num": q.layers_num}
        q.activation_quantize(cases.calib_batches(3, shape, seed=tn.G24_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        got["feat_table"] = open(os.path.join(wd, "feat.table")).read()
        q.weight_quantize()
        got["weight_table"] = open(os.path.join(wd, "weight.table")).read()
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table"):
            assert got[key] == ref[key], key
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(cases.seed_model(tn.g24_net(), base_seed=tn.G24_SEED).eval())
        info = rec.get_quantity_information()
        assert sorted(info.keys()) == ref["recon_layers"]
        assert {k: {kk: vv for kk, vv in v.items() if kk != "layer"} for k, v in info.items()} == ref["quantity_information"]
        with topdown_doubles.installed() as nat, _Spy(nat) as spy:
            net = rec.ReconModel(info, os.path.join(wd, "recon.pth"))
            x = cases.fixed_input(shape, seed=tn.G24_INPUT_SEED)
            np.testing.assert_array_equal(x.numpy(), arrays["x"])
            with torch.no_grad():
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                off = resident.enable(net, x, concat=True)
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                off_plans = _plans(net)
                assert not spy.up
                on = resident.enable(net, x, concat=True, topdown=True)
                spy.clear()
                np.testing.assert_array_equal(net(x).numpy(), arrays["logits_recon"])
                np.testing.assert_array_equal(net(x[:1]).numpy(), arrays["logits_recon"][:1])
            plans = _plans(net)
            assert on["topdown_adds"] == 2 and on["topdown_sum_sources"] == 1 and not plans.topdown_left, (on, plans.topdown_left)
            assert off["fp32_outputs"] - on["fp32_outputs"] == 2 and len(spy.up) == 4 and not spy.moved
            assert off_plans["Eltwise1"].emit_f32 and "Eltwise2" not in off_plans
            e1 = plans["Eltwise1"]                              # the sum read by the second upsampling and by out3
            assert not e1.emit_f32 and e1.want_wide and e1.narrow_bit == info["out3"]["input_bit"]
            assert not plans["Eltwise2"].emit_f32 and plans["up1"].defer and plans["up2"].defer


# ---------------------------------------------------------------- 5. the random family
SEEDS = list(range(40))
ADMITTED = (92, 79, 44)          # upsamplings of the forty models, those the rule admits, those among them that read a sum


def test_the_random_family_by_construction():
    ups = [u for seed in SEEDS for u in tn.RandomTopDown(seed).ups]
    assert all(len(tn.RandomTopDown(seed).ups) >= 1 for seed in SEEDS)
    got = (len(ups), sum(1 for _n, ok, _s in ups if ok), sum(1 for _n, ok, s in ups if ok and s))
    print("random family: %d upsamplings in front of an add, %d admitted, %d of them over a sum" % got)
    assert got == ADMITTED
    assert set(f for seed in SEEDS for f in tn.RandomTopDown(seed).factors) == {2, 4}


@pytest.mark.parametrize("seed", SEEDS)
def test_random_topdown(seed):
    """Each drawn model under `concat`, `concat + topdown` and all ten switches: exact logits, and with `topdown` every
    upsampling the rule admits is planned (a condition, not a measurement), every other one is named in topdown_left."""
    from common.quantity import resident
    with topdown_doubles.installed():
        net = tn.RandomTopDown(seed).eval()
        x = net.example()
        with torch.no_grad():
            plain = net(x)
        want = sum(1 for _n, ok, _s in net.ups if ok)
        a = resident.enable(net, x, concat=True)
        assert "topdown_adds" not in a
        _check_forwards(net, x, plain)
        for kw in (dict(concat=True, topdown=True), ALL_TEN):
            on = resident.enable(net, x, **kw)
            plans = _plans(net)
            assert on["topdown_adds"] == want, (on, net.ups, plans.topdown_left)
            assert on["topdown_sum_sources"] == sum(1 for _n, ok, s in net.ups if ok and s)
            for name, ok, _s in net.ups:
                assert (name in plans.topdown_left) == (not ok), (name, plans.topdown_left)
                assert (name in plans and plans[name].defer and isinstance(net.get_submodule(name).__dict__.get("forward"),
                                                                           resident._UpsampleTopDown)) == ok, name
            _check_forwards(net, x, plain)
        resident.disable(net)
        _check_forwards(net, x, plain)


# ---------------------------------------------------------------- 6. the mixed family with the tenth switch
@pytest.mark.parametrize("index", [i for i, _seed in mn.family()][:8])
def test_random_mixed_nets_with_all_ten_switches(index, oracle):
    from common.quantity import resident
    seed = dict(mn.family())[index]
    with topdown_doubles.installed():
        _info, (net,) = mn.calibrated(index, seed, [topdown_doubles.installed])
        x, x2 = mn.inputs(net, index, seed)
        with torch.no_grad():
            want = [net(x).clone(), net(x2).clone()]
        nine = resident.enable(net, x, **{k: v for k, v in ALL_TEN.items() if k != "topdown"})
        ten = resident.enable(net, x, **ALL_TEN)
        assert set(ten) == set(nine) | {"topdown_adds", "topdown_sum_sources"}
        with torch.no_grad():
            assert torch.equal(net(x), want[0]) and torch.equal(net(x2), want[1])
        resident.disable(net)
        with torch.no_grad():
            assert torch.equal(net(x), want[0])


# ---------------------------------------------------------------- 7. the model file
def test_resnet50_fpn_needs_a_multiple_of_32_and_plans_its_pathway():
    from model.fpn.ResNetFPN_fabu import ResNet50FPN
    for size in (0, 16, 48, 225):
        with pytest.raises(ValueError):
            ResNet50FPN(10, size)
    net = ResNet50FPN(10, 64)
    ups = [m for m in net.modules() if isinstance(m, nn.Upsample)]
    assert len(ups) == 2 and all(type(m) is nn.UpsamplingNearest2d for m in ups)
    assert sum(type(m).__name__ == "Eltwise" for m in net.modules()) >= 16 + 2
    with torch.no_grad():
        out = net.eval()(torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(0)))
    assert tuple(out.shape) == (1, 10)
