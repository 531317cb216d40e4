"""resident.enable(..., avgpool=True, sums=True) on the MI355X: windowed average pools over NewAdd sums on fq_avgpool_i16_nhwc
inside ResNet-D-shaped nets, golden G23 and ResNet-50-D calibrated end to end, eagerly and as one HIP graph.  Everything is
integers: every comparison is exact.   pytest -m gpu"""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import avgpool_nets as an
import cases
import sum_pool_nets as sn
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


# (net, name of the pool, name of the sum it reads, fusions that must be in the summary with the switch on)
NETS = {
    "add_source": (lambda: an.PoolNet(mode="add_source"), "pool", "add", {}),
    "identity": (lambda: sn.DBlockNet(), "d.pool", "f1.add", dict(fused_block_tails=0, fused_projections=0)),
    "skip": (lambda: sn.DBlockNet(skip=True), "d.pool", "f1.add", {}),
    "tail": (lambda: sn.DBlockNet(front="tail"), "d.pool", "f2.add", dict(fused_block_tails=2)),
    "proj": (lambda: sn.DBlockNet(front="proj"), "d.pool", "f1.add", dict(fused_projections=1)),
    "pool_3x3": (lambda: sn.DBlockNet(pool=nn.AvgPool2d(3, 2, 1, count_include_pad=False)), "d.pool", "f1.add", {}),
    "relu_behind": (lambda: sn.SumPoolNet(relu_front=False, relu_behind=True), "pool", "add", {}),
    "two_readers": (lambda: sn.SumPoolNet(pool=nn.AvgPool2d(3, 1, 1, count_include_pad=False), read_bits=(4, 4)), "pool", "add", {}),
    "operands_on_two_grids": (lambda: sn.SumPoolNet(sum_bits=(3, 6), read_bits=(5,)), "pool", "add", {}),
    "shift_8": (lambda: sn.SumPoolNet(sum_bits=(-1, -1), read_bits=(8,)), "pool", "add", {}),
    "shift_minus_8": (lambda: sn.SumPoolNet(sum_bits=(8, 8), read_bits=(0,)), "pool", "add", {}),
}


@pytest.mark.parametrize("tag", sorted(NETS))
def test_modules_with_and_without_the_switch(nat, tag):
    from common.quantity import resident
    make, pool, src, fusions = NETS[tag]
    net, x = make().cuda().eval(), sn.example().cuda()
    with torch.no_grad():
        plain = net(x)
    off = resident.enable(net, x, avgpool=True)                                 # without the switch: the sum leaves as fp32
    plans = resident.describe(net)
    assert "resident_sum_avgpools" not in off and off["resident_avgpools"] == 0 and pool not in plans and plans[src].emit_f32
    _check_forwards(net, x, plain)

    on = resident.enable(net, x, avgpool=True, sums=True)                       # verify=True
    plans = resident.describe(net)
    assert on["resident_sum_avgpools"] == 1 and on["fp32_outputs"] == off["fp32_outputs"] - 1, (off, on)
    assert {k: on[k] for k in fusions} == fusions and not plans.avgpool_left, (on, plans.avgpool_left)
    assert not plans[src].emit_f32 and plans[src].want_wide and not plans[pool].emit_f32 and plans[pool].emit_int
    assert isinstance(net.get_submodule(pool).__dict__["forward"], resident._AvgPoolWindowResident)
    calls = []
    real = nat.avgpool_i16_nhwc
    nat.avgpool_i16_nhwc = lambda *a, **k: (calls.append(a[0].dtype), real(*a, **k))[1]
    try:
        _check_forwards(net, x, plain)
    finally:
        nat.avgpool_i16_nhwc = real
    assert calls == [torch.int16] * 3
    resident.disable(net)
    assert not resident.describe(net) and all("forward" not in m.__dict__ for m in net.modules())
    _check_forwards(net, x, plain)


@pytest.mark.parametrize("tag", ["two_bits", "shift_9", "window_9x9", "ceil_mode"])
def test_declined_plans_keep_the_fp32_form(nat, tag):
    from common.quantity import resident
    make = {"two_bits": lambda: sn.SumPoolNet(read_bits=(4, 3)), "shift_9": lambda: sn.SumPoolNet(sum_bits=(-1, -1), read_bits=(9,)),
            "window_9x9": lambda: sn.SumPoolNet(pool=nn.AvgPool2d(9, 1, 4)), "ceil_mode": lambda: sn.SumPoolNet(pool=nn.AvgPool2d(2, ceil_mode=True))}[tag]
    net, x = make().cuda().eval(), sn.example().cuda()
    with torch.no_grad():
        plain = net(x)
    on = resident.enable(net, x, avgpool=True, sums=True)
    plans = resident.describe(net)
    assert on["resident_sum_avgpools"] == 0 and "pool" not in plans and "forward" not in net.pool.__dict__, (on, plans)
    assert plans["add"].emit_f32 and set(plans.avgpool_left) == {"pool"}
    _check_forwards(net, x, plain)


# ---------------------------------------------------------------- golden G23
def test_g23_logits_equal_the_reference_with_the_switch_on(nat, oracle, golden_dir):
    """The reference's ReconModel logits of sum_pool_nets.g23_net (CPU, fixed input) against the integer-simulation model on the
    HIP kernels: plain, with avgpool=True and with sums=True, bit for bit.  The tables come from the oracle-backed CPU calibration,
    which tests/test_sum_pool_plan_cpu.py pins to the reference's byte for byte."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    with open(os.path.join(golden_dir, "g23_resnetd_net.json")) as fh:
        ref = json.load(fh)
    want = np.load(os.path.join(golden_dir, "g23_resnetd_net.npz"))["logits_recon"]
    shape = sn.G23_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(cases.seed_model(sn.g23_net(), base_seed=sn.G23_SEED).eval())
        q.activation_quantize(cases.calib_batches(3, shape, seed=sn.G23_CALIB_SEED))
        q.weight_quantize()
        q.rewrite_weight()
        wd = os.path.join(tmp, "test", "workdir")
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(cases.seed_model(sn.g23_net(), base_seed=sn.G23_SEED).eval())
        net = rec.ReconModel(rec.get_quantity_information(), os.path.join(wd, "recon.pth")).cuda()
        x = cases.fixed_input(shape, seed=sn.G23_INPUT_SEED).cuda()
        with torch.no_grad():
            np.testing.assert_array_equal(net(x).cpu().numpy(), want)
            off = resident.enable(net, x, avgpool=True)
            np.testing.assert_array_equal(net(x).cpu().numpy(), want)
            on = resident.enable(net, x, avgpool=True, sums=True)
            np.testing.assert_array_equal(net(x).cpu().numpy(), want)
            np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), want[:1])
        assert on["resident_sum_avgpools"] == 2 and off["fp32_outputs"] - on["fp32_outputs"] == 2, (off, on)


# ---------------------------------------------------------------- ResNet-50-D calibrated end to end
def _resnet50d(size):
    from common.quantity import merge_bn
    from model.resnetd.ResNetD_fabu import ResNet50D
    # gamma_scale 0.5, as the ResNet-50 tests at 224 use it: with 1.0 the activations of this seeded model grow through the sixteen
    # adds until the calibrated output bits are negative and every logit quantises to zero
    return merge_bn(cases.seed_model(ResNet50D(num_classes=10, input_size=size), gamma_scale=0.5).eval())


STAGE_SUMS = ("layer1.2.Eltwise", "layer2.3.Eltwise", "layer3.5.Eltwise")      # the sums in front of stages 2, 3 and 4


@pytest.mark.parametrize("size", [32, 64])
def test_calibrated_resnet50d_with_the_sum_pool_plan(nat, size, tmp_path):
    """At 64 x 64 the three sums in front of stages 2, 3 and 4 go from emit_f32 to integer-only.  At 32 x 32 the last shortcut
    pool's 2 x 2 window is the whole plane in front of stage 4: without the switch the whole-plane path (fq_avgpool_global_nhwc)
    already reads that sum's exact integers, so only the first two sums leave as fp32 there; with the switch all three pools run
    on fq_avgpool_i16_nhwc at either size."""
    from common.quantity import resident
    from tools import Quantity, Reconstruction
    shape = (4, 3, size, size)
    with product_workdir(input_shape="1,3,%d,%d" % (size, size), device="gpu", max_cali_img_num=1) as tmp:
        wd = os.path.join(tmp, "test", "workdir")
        q = Quantity(_resnet50d(size).cuda())
        q.activation_quantize(cases.calib_batches(2, shape))
        q.weight_quantize()
        rec = Reconstruction(_resnet50d(size))
        net = rec.ReconModel(rec.get_quantity_information(), os.path.join(wd, "recon_d.pth")).cuda()
        x = cases.fixed_input(shape).cuda()
        with torch.no_grad():
            plain = net(x)
        assert float(plain.std()) > 0
        off = resident.enable(net, x, avgpool=True)
        off_plans = resident.describe(net)
        with torch.no_grad():
            off_out = net(x)
        on = resident.enable(net, x, avgpool=True, sums=True)                   # verify=True
        plans = resident.describe(net)
        print("resnet50d %d: off %s; on %s" % (size, off, on))
        assert off["resident_avgpools"] == 0 and "resident_sum_avgpools" not in off
        assert on["resident_sum_avgpools"] == 3 and on["resident_avgpools"] == 3 and not plans.avgpool_left, plans.avgpool_left
        whole_plane = 1 if size == 32 else 0
        assert on["fp32_outputs"] == off["fp32_outputs"] - (3 - whole_plane) and on["resident_convs"] == off["resident_convs"]
        assert on["resident_pools"] == off["resident_pools"] - whole_plane == 2          # the max-pool and the head's pool
        for name in STAGE_SUMS:
            assert off_plans[name].emit_f32 == (not (whole_plane and name == STAGE_SUMS[2])), name
            assert not plans[name].emit_f32 and plans[name].emit_int and plans[name].want_wide, name
        for stage in ("layer2", "layer3", "layer4"):
            pool = net.get_submodule(stage + ".0.downsample.0")
            assert isinstance(pool, nn.AvgPool2d) and isinstance(pool.__dict__["forward"], resident._AvgPoolWindowResident)
        assert not isinstance(net.layer1[0].downsample[0], nn.AvgPool2d)         # stage 1's projection has no pool
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
def test_hipgraph_capture_of_a_sum_pool_plan_replays_another_input(nat):
    """A replay on a DIFFERENT input must give that input's logits."""
    from common.quantity import resident
    for make in (sn.DBlockNet, lambda: sn.DBlockNet(front="tail"), lambda: sn.SumPoolNet(relu_front=False, relu_behind=True)):
        net = make().cuda().eval()
        x, x2 = sn.example(seed=1).cuda(), sn.example(seed=2).cuda() * 1.5
        with torch.no_grad():
            want, want2 = tuple(t.clone() for t in _tuple(net(x))), tuple(t.clone() for t in _tuple(net(x2)))
        assert not _same(want, want2)
        summary = resident.enable(net, x, avgpool=True, sums=True)
        assert summary["resident_sum_avgpools"] == 1
        graphed = resident.GraphedForward(net, x)
        assert _same(graphed(x), want)
        assert _same(graphed(x2), want2)
        assert _same(graphed(x), want)
        with torch.no_grad():
            assert _same(net(x2), want2)
