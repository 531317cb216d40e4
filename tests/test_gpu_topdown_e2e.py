"""resident.enable(..., concat=True, topdown=True) on the MI355X: NewAdds that read an operand through a nearest upsampling on
fq_add_up_resident inside FPN-shaped nets, golden G24 and ResNet-50-FPN calibrated end to end, eagerly and as one HIP graph.
Everything is integers: every comparison is exact.   pytest -m gpu"""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import cases
import topdown_nets as tn
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


def _tuple(t):
    return t if isinstance(t, tuple) else (t,)


def _same(a, b):
    a, b = _tuple(a), _tuple(b)
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def _check_forwards(net, x, plain):
    with torch.no_grad():
        assert _same(net(x), plain)
        assert _same(net(x[:1]), tuple(p[:1] for p in _tuple(plain)))
        assert _same(net(torch.flip(x, dims=[0])), tuple(torch.flip(p, dims=[0]) for p in _tuple(plain)))


# tag: (net arguments, topdown_adds, topdown_sum_sources, names in topdown_left)
NETS = {
    "plain": (dict(), 2, 1, ()),
    "relu_behind_the_sums": (dict(relu_sum=True), 2, 1, ()),
    "upsampled_operand_first": (dict(swap=True), 2, 1, ()),
    "factor_4": (dict(factor=4), 2, 1, ()),
    "operands_on_three_grids": (dict(bits=(3, 5, 6), read_bits=(2, 6)), 2, 1, ()),
    "grid_8_and_negative_bits": (dict(bits=(-1, 8, 2), read_bits=(0, 7)), 2, 1, ()),
    "relu_behind_the_upsampling": (dict(mode="relu_behind"), 1, 0, ("up2",)),
    "module_called_twice": (dict(mode="twice"), 0, 0, ("up1",)),
    "second_reader_over_a_sum": (dict(mode="extra_reader"), 1, 0, ("up2",)),
    "second_reader_over_int8": (dict(mode="extra_reader_int8"), 1, 1, ("up1",)),
    "both_operands_upsampled": (dict(mode="both_up"), 1, 1, ("up1", "up1b")),
    "bilinear": (dict(up=lambda step: nn.Upsample(scale_factor=2, mode="bilinear")), 0, 0, ("up1", "up2")),
}


@pytest.mark.parametrize("tag", sorted(NETS))
def test_modules_with_and_without_the_switch(nat, tag):
    from common.quantity import resident
    kw, n_adds, n_sums, left = NETS[tag]
    net = tn.TopDownNet(**kw).cuda().eval()
    x = net.example().cuda()
    with torch.no_grad():
        plain = net(x)
    off = resident.enable(net, x, concat=True)
    assert "topdown_adds" not in off and not resident.describe(net).topdown_left
    _check_forwards(net, x, plain)

    on = resident.enable(net, x, concat=True, topdown=True)                     # verify=True
    plans = resident.describe(net)
    assert on["topdown_adds"] == n_adds and on["topdown_sum_sources"] == n_sums and set(plans.topdown_left) == set(left), (on, plans.topdown_left)
    if n_adds == 2:
        assert on["fp32_outputs"] == off["fp32_outputs"] - 2
        assert not plans["add1"].emit_f32 and plans["add1"].want_wide and not plans["add2"].emit_f32
        assert plans["up1"].defer and plans["up2"].defer
    calls = []
    real = nat.add_up_resident
    nat.add_up_resident = lambda *a, **k: (calls.append((a[0].dtype, a[2].dtype, a[4])), real(*a, **k))[1]
    try:
        _check_forwards(net, x, plain)
    finally:
        nat.add_up_resident = real
    assert len(calls) == 3 * n_adds
    if n_adds == 2:
        assert calls[:2] == [(torch.int8, torch.int8, net.factor), (torch.int8, torch.int16, net.factor)]
    resident.disable(net)
    assert not resident.describe(net) and all("forward" not in m.__dict__ for m in net.modules())
    _check_forwards(net, x, plain)


def test_run_time_fallbacks_on_the_device(nat):
    """A plan grid that disagrees: the int8 payload goes through the stand-alone upsampling launch, the int16 payload through
    the module's own forward on the de-quantised coarse tensor; the values are the planned path's."""
    from common.quantity import resident
    net = tn.TopDownNet().cuda().eval()
    x = net.example().cuda()
    resident.enable(net, x, concat=True, topdown=True)
    with torch.no_grad():
        c2 = net.r0(net.stem(x))
        c3 = net.r1(net.d1(c2))
        lat3, lat2, p4 = net.l3(c3), net.l2(c2), net.l4(net.r2(net.d2(c3)))
        s3 = net.add1(lat3, net.up1(p4))
        want3, want2 = s3.to_f32(), net.o2(net.add2(lat2, net.up2(s3)))
        for add, lat, top, up in ((net.add1, lat3, p4, net.up1), (net.add2, lat2, s3, net.up2)):
            plan = add.__dict__["_resident"]
            plan.grid += 1
            try:
                out = add(lat, up(top))
            finally:
                plan.grid -= 1
            assert isinstance(out, torch.Tensor) and out.dtype == torch.float32
            assert torch.equal(out, want3) if add is net.add1 else torch.equal(net.o2(out), want2)


# ---------------------------------------------------------------- golden G24
def test_g24_logits_equal_the_reference_with_the_switch_on(nat, oracle, golden_dir):
    """The reference's ReconModel logits of topdown_nets.g24_net (CPU, fixed input) against the integer-simulation model on the
    HIP kernels: plain, with concat=True and with topdown=True, bit for bit.  The tables come from the oracle-backed CPU
    calibration, which tests/test_topdown_plan_cpu.py pins to the reference's byte for byte."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    with open(os.path.join(golden_dir, "g24_topdown_net.json")) as fh:
        ref = json.load(fh)
    want = np.load(os.path.join(golden_dir, "g24_topdown_net.npz"))["logits_recon"]
    shape = tn.G24_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(cases.seed_model(tn.g24_net(), base_seed=tn.G24_SEED).eval())
        q.activation_quantize(cases.calib_batches(3, shape, seed=tn.G24_CALIB_SEED))
        q.weight_quantize()
        q.rewrite_weight()
        wd = os.path.join(tmp, "test", "workdir")
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(cases.seed_model(tn.g24_net(), base_seed=tn.G24_SEED).eval())
        net = rec.ReconModel(rec.get_quantity_information(), os.path.join(wd, "recon.pth")).cuda()
        x = cases.fixed_input(shape, seed=tn.G24_INPUT_SEED).cuda()
        with torch.no_grad():
            np.testing.assert_array_equal(net(x).cpu().numpy(), want)
            off = resident.enable(net, x, concat=True)
            np.testing.assert_array_equal(net(x).cpu().numpy(), want)
            on = resident.enable(net, x, concat=True, topdown=True)
            np.testing.assert_array_equal(net(x).cpu().numpy(), want)
            np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), want[:1])
        assert on["topdown_adds"] == 2 and on["topdown_sum_sources"] == 1 and off["fp32_outputs"] - on["fp32_outputs"] == 2, (off, on)


# ---------------------------------------------------------------- ResNet-50-FPN calibrated end to end
def _resnet50fpn(size):
    from common.quantity import merge_bn
    from model.fpn.ResNetFPN_fabu import ResNet50FPN
    # gamma_scale 0.5, as the ResNet-50 tests use it: with 1.0 the activations of this seeded model grow through the sixteen adds
    return merge_bn(cases.seed_model(ResNet50FPN(num_classes=10, input_size=size), gamma_scale=0.5).eval())


def test_calibrated_resnet50_fpn_with_the_topdown_plan(nat, tmp_path):
    """64 x 64, batch 2: both top-down adds run on fq_add_up_resident, the second over the int16 sum of the first; that sum goes
    from emit_f32 to integer-only (wide for the upsampling, narrow for its 3x3 output convolution)."""
    from common.quantity import resident
    from tools import Quantity, Reconstruction
    size, shape = 64, (2, 3, 64, 64)
    with product_workdir(input_shape="1,3,%d,%d" % (size, size), device="gpu", max_cali_img_num=1) as tmp:
        wd = os.path.join(tmp, "test", "workdir")
        q = Quantity(_resnet50fpn(size).cuda())
        q.activation_quantize(cases.calib_batches(2, shape))
        q.weight_quantize()
        rec = Reconstruction(_resnet50fpn(size))
        net = rec.ReconModel(rec.get_quantity_information(), os.path.join(wd, "recon_fpn.pth")).cuda()
        x = cases.fixed_input(shape).cuda()
        with torch.no_grad():
            plain = net(x)
        assert float(plain.std()) > 0
        off = resident.enable(net, x, concat=True)
        off_plans = resident.describe(net)
        with torch.no_grad():
            off_out = net(x)
        on = resident.enable(net, x, concat=True, topdown=True)                 # verify=True
        plans = resident.describe(net)
        print("resnet50fpn %d: off %s; on %s" % (size, off, on))
        assert "topdown_adds" not in off and on["topdown_adds"] == 2 and on["topdown_sum_sources"] == 1 and not plans.topdown_left
        assert on["fp32_outputs"] == off["fp32_outputs"] - 2 and on["resident_convs"] == off["resident_convs"]
        assert on["resident_upsamples"] == off["resident_upsamples"] + 1 == 2 and on["resident_adds"] == off["resident_adds"] + 1
        assert off_plans["Eltwise4"].emit_f32 and "Eltwise3" not in off_plans and "up4" not in off_plans
        e4, e3 = plans["Eltwise4"], plans["Eltwise3"]
        assert not e4.emit_f32 and e4.want_wide and e4.narrow_bit == net.output4.input_bit and e4.fuse_arg is None
        assert not e3.emit_f32 and e3.resident_add and e3.narrow_bit == net.output3.input_bit
        assert plans["up5"].defer and plans["up4"].defer and plans["up4"].narrow_bit == e4.grid
        for name in ("up5", "up4"):
            assert isinstance(net.get_submodule(name).__dict__["forward"], resident._UpsampleTopDown)
        with torch.no_grad():
            assert torch.equal(net(x), plain) and torch.equal(off_out, plain)
            assert torch.equal(net(x[:1]), plain[:1])
            assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
        path = str(tmp_path / "planned.pth")                                    # save / load round trip of the planned model
        torch.save(net, path)
        again = torch.load(path, weights_only=False)
        assert resident.is_enabled(again) and len(resident.describe(again)) == len(plans)
        with torch.no_grad():
            assert torch.equal(again(x), plain)
        resident.disable(net)
        assert not resident.describe(net) and all("forward" not in m.__dict__ for m in net.modules())
        with torch.no_grad():
            assert torch.equal(net(x), plain)


# ---------------------------------------------------------------- HIP-graph capture of the plan
def test_hipgraph_capture_of_a_topdown_plan_replays_another_input(nat):
    """A replay on a DIFFERENT input must give that input's outputs."""
    from common.quantity import resident
    for kw in (dict(), dict(relu_sum=True, swap=True), dict(factor=4), dict(mode="extra_reader")):
        net = tn.TopDownNet(**kw).cuda().eval()
        x, x2 = net.example(seed=1).cuda(), net.example(seed=2).cuda() * 1.5
        with torch.no_grad():
            want, want2 = tuple(t.clone() for t in _tuple(net(x))), tuple(t.clone() for t in _tuple(net(x2)))
        assert not _same(want, want2)
        summary = resident.enable(net, x, concat=True, topdown=True)
        assert summary["topdown_adds"] >= 1
        graphed = resident.GraphedForward(net, x)
        assert _same(graphed(x), want)
        assert _same(graphed(x2), want2)
        assert _same(graphed(x), want)
        with torch.no_grad():
            assert _same(net(x2), want2)
