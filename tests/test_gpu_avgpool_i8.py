"""Windowed average pooling of resident int8 activations (fq_avgpool_i8_nhwc, csrc/fq_avgpool_i8.hip) against the rule of
include/fq.h in NumPy float32 (avgpool_nets.numpy_rule, which tests/test_avgpool_plan_cpu.py holds against torch's own chain), and
resident.enable(..., avgpool=True) on Inception / transition style nets and calibrated models.  Everything is integers: every
comparison is exact.   pytest -m gpu"""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import avgpool_nets as an
import cases
import depthwise_nets as dn
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu

FQ_OK, FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED = 0, -1, -4
SENTINEL, GUARD = 0x5A, 64


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


# ---------------------------------------------------------------- 1. the kernel against the rule
def _run_in_view(nat, x_dev, want, C, kernel, stride, padding, cip, shift, relu):
    """The output is a view inside a larger buffer: sentinel bytes in front of and behind it must survive."""
    buf = torch.full((GUARD + want.size + GUARD,), SENTINEL, dtype=torch.int8, device="cuda")
    view = buf[GUARD:GUARD + want.size].view(want.shape)
    assert view.data_ptr() % 16 == 0
    got = nat.avgpool_i8_nhwc(x_dev, C, kernel, stride, padding, cip, shift, relu, out=view)
    assert got is view
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + want.size:] == SENTINEL).all()
    return host[GUARD:GUARD + want.size].reshape(want.shape)


@pytest.mark.parametrize("case", an.KERNEL_CASES, ids=an.case_arg)
def test_avgpool_kernel_vs_the_rule(nat, case):
    rng = np.random.default_rng(sum((i + 1) * v for i, v in enumerate(case)))
    C, kernel, stride, padding = case[3], case[4:6], case[6:8], case[8:10]
    for kind in ("random", "max", "min"):
        x = an.source(rng, case, kind)
        assert x[..., C:].all() or C == x.shape[-1]                            # garbage in the source's padding channels
        x_dev = torch.from_numpy(x).cuda()
        for cip in (False, True):
            for relu in (False, True):
                for shift in an.SHIFTS:
                    want = an.numpy_rule(x, C, kernel, stride, padding, cip, shift, relu)
                    got = _run_in_view(nat, x_dev, want, C, kernel, stride, padding, cip, shift, relu)
                    np.testing.assert_array_equal(got, want, err_msg=str((kind, cip, relu, shift)))
                    assert not got[..., C:].any()                               # zeros in the output's
        own = nat.avgpool_i8_nhwc(x_dev, C, kernel, stride, padding, True, 0, False)           # ... and the allocating form
        assert tuple(own.shape) == (case[0],) + an.out_plane(case) + (an.pad16(C),)
        np.testing.assert_array_equal(own.cpu().numpy(), an.numpy_rule(x, C, kernel, stride, padding, True, 0, False))
        np.testing.assert_array_equal(x_dev.cpu().numpy(), x)                                   # the source is only read


def test_the_case_list_covers_what_it_claims():
    cs = an.KERNEL_CASES
    assert {c[3] for c in cs} == {1, 16, 19, 100} and {c[0] for c in cs} == {1, 3}
    assert {c[6] for c in cs} >= {1, 2, 3} and {(c[1], c[2]) for c in cs} >= {(1, 1), (2, 2), (5, 7), (9, 11)}
    assert (1, 1, 1, 1, 3, 3, 1, 1, 1, 1) in cs and any(c[4] > c[1] + c[8] for c in cs)                 # one tap; window larger than the image
    assert any(c[4:10] == (2, 2, 2, 2, 0, 0) and c[1] % 2 and c[2] % 2 for c in cs)                    # last row and column dropped
    assert any(c[4:10] == (2, 3, 1, 2, 1, 1) for c in cs) and any(c[4:10] == (7, 7, 1, 1, 3, 3) for c in cs)
    assert any(c[4:10] == (8, 8, 8, 8, 0, 0) for c in cs) and set(an.SHIFTS) == {-8, -1, 0, 1, 8}
    # S = +-8192 at the cap, and saturation at a positive shift
    cap = (1, 16, 8, 19, 8, 8, 8, 8, 0, 0)
    lo = an.numpy_rule(an.source(None, cap, "min"), 19, (8, 8), (8, 8), (0, 0), True, 0, False)
    hi = an.numpy_rule(an.source(None, cap, "max"), 19, (8, 8), (8, 8), (0, 0), True, 1, False)
    assert (lo[..., :19] == -128).all() and (hi[..., :19] == 127).all()


def test_ties_round_half_to_even(nat):
    x = an.tie_source()
    x_dev = torch.from_numpy(x).cuda()
    for shift, want in ((0, [[0, 2, 2], [0, -2, -2], [1, 3, -1]]), (-1, [[0, 1, 1], [0, -1, -1], [0, 2, 0]])):
        rule = an.numpy_rule(x, 16, (2, 2), (2, 2), (0, 0), True, shift, False)
        assert rule[0, :, :, 0].tolist() == want                                # half away from zero would give 1, 2, 3, -1, ...
        got = nat.avgpool_i8_nhwc(x_dev, 16, (2, 2), (2, 2), (0, 0), True, shift, False).cpu().numpy()
        np.testing.assert_array_equal(got, rule)


def test_more_chunks_than_lanes(nat):
    """540 800 chunks on 2048 x 256 lanes: the first 16 512 lanes take a second chunk."""
    case = an.STRIDE_LOOP_CASE
    assert case[0] * case[1] * case[2] * (case[3] // 16) > 2048 * 256
    x = an.source(np.random.default_rng(5), case)
    got = nat.avgpool_i8_nhwc(torch.from_numpy(x).cuda(), case[3], (3, 3), (1, 1), (1, 1), False, 1, True).cpu().numpy()
    np.testing.assert_array_equal(got, an.numpy_rule(x, case[3], (3, 3), (1, 1), (1, 1), False, 1, True))


# ---------------------------------------------------------------- 2. what the entry point declines
def _raw(nat, x, y, N, H, W, C, Cpad, kh, kw, sh, sw, ph, pw, cip=1, shift=0, relu=0):
    ptr = lambda t: None if t is None else (ctypes.c_void_p(t) if isinstance(t, int) else ctypes.c_void_p(t.data_ptr()))
    return nat.lib().fq_avgpool_i8_nhwc(ptr(x), ptr(y), N, H, W, C, Cpad, kh, kw, sh, sw, ph, pw, cip, shift, relu, None)


def test_declined_cases_and_argument_errors(nat):
    """By return code only: every buffer is large enough for any geometry that could be launched, and nothing may be launched."""
    x = torch.zeros(2, 16, 16, 32, dtype=torch.int8, device="cuda")
    y = torch.full((2, 16, 16, 32), 5, dtype=torch.int8, device="cuda")
    sup = nat.lib().fq_avgpool_i8_nhwc_supported
    ok = (2, 16, 16, 20, 32, 3, 3, 1, 1, 1, 1)
    bad = FQ_ERR_INVALID_ARG
    assert _raw(nat, None, y, *ok) == bad and _raw(nat, x, None, *ok) == bad                             # null pointers
    assert _raw(nat, x.data_ptr() + 4, y, 1, 8, 8, 16, 16, 3, 3, 1, 1, 1, 1) == bad                       # misaligned source
    assert _raw(nat, x, y.data_ptr() + 8, 1, 8, 8, 16, 16, 3, 3, 1, 1, 1, 1) == bad                       # misaligned output
    assert _raw(nat, x, y, -1, 16, 16, 20, 32, 3, 3, 1, 1, 1, 1) == bad                                   # sizes
    assert _raw(nat, x, y, 2, 0, 16, 20, 32, 3, 3, 1, 1, 1, 1) == bad and _raw(nat, x, y, 2, 16, 0, 20, 32, 3, 3, 1, 1, 1, 1) == bad
    assert _raw(nat, x, y, 2, 16, 16, 0, 32, 3, 3, 1, 1, 1, 1) == bad and _raw(nat, x, y, 2, 16, 16, 20, 0, 3, 3, 1, 1, 1, 1) == bad
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 0, 3, 1, 1, 0, 1) == bad and _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 0, 1, 1, 1, 0) == bad    # kernel
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 3, 0, 1, 1, 1) == bad and _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 3, 1, -1, 1, 1) == bad   # stride
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 3, 1, 1, -1, 1) == bad                                   # negative padding
    assert _raw(nat, x, y, 2, 16, 16, 33, 32, 3, 3, 1, 1, 1, 1) == bad                                    # C > Cpad
    assert _raw(nat, x, y, 2, 16, 16, 20, 24, 3, 3, 1, 1, 1, 1) == bad                                    # Cpad % 16
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 3, 1, 1, 2, 1) == bad and _raw(nat, x, y, 2, 16, 16, 20, 32, 3, 3, 1, 1, 1, 2) == bad    # 2 pad > kernel
    assert _raw(nat, x, y, 2, 4, 16, 20, 32, 7, 3, 2, 1, 1, 1) == bad and _raw(nat, x, y, 2, 16, 4, 20, 32, 3, 7, 1, 2, 1, 1) == bad      # P < 1, Q < 1
    un = FQ_ERR_UNSUPPORTED
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 9, 9, 1, 1, 4, 4) == un and sup(9, 9, 1, 1, 4, 4, 0) == 0   # 81 taps
    assert _raw(nat, x, y, 2, 16, 16, 20, 32, 5, 13, 1, 1, 0, 0) == un and sup(5, 13, 1, 1, 0, 0, 0) == 0  # 65 taps
    assert _raw(nat, x, y, *ok, shift=9) == un and _raw(nat, x, y, *ok, shift=-9) == un
    assert sup(3, 3, 1, 1, 1, 1, 9) == 0 and sup(3, 3, 1, 1, 1, 1, -9) == 0
    assert _raw(nat, x, y, 1, 32768, 32768, 16, 16, 2, 2, 2, 2, 0, 0) == un                               # a source of 2^34 bytes
    assert _raw(nat, x, y, 1, 32768, 4096, 16, 16, 1, 1, 1, 1, 0, 0) == un                                # ... of 2^31 bytes
    assert sup(3, 3, 1, 1, 1, 1, 0) == 1 and sup(8, 8, 8, 8, 4, 4, 8) == 1 and sup(2, 3, 1, 2, 1, 1, -8) == 1
    assert sup(3, 3, 1, 1, 2, 1, 0) == 0 and sup(0, 3, 1, 1, 0, 0, 0) == 0 and sup(3, 3, 0, 1, 0, 0, 0) == 0 and sup(3, 3, 1, 1, -1, 0, 0) == 0
    assert _raw(nat, None, None, 0, 16, 16, 20, 32, 3, 3, 1, 1, 1, 1) == FQ_OK                            # N == 0
    torch.cuda.synchronize()
    assert bool((y == 5).all())                                                                           # nothing was launched
    assert _raw(nat, x, y, *ok) == FQ_OK
    torch.cuda.synchronize()
    assert not bool((y == 5).any())


# ---------------------------------------------------------------- 3. modules
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


NETS = {
    "inception_block": lambda: an.InceptionBlockNet(),
    "transition": lambda: an.PoolNet(),
    "relu_behind": lambda: an.PoolNet(relu_behind=True),
    "two_readers": lambda: an.PoolNet(pool=nn.AvgPool2d(3, 1, 1, count_include_pad=False), read_bits=(4, 4)),
    "reader_at_another_bit": lambda: an.PoolNet(read_bits=(3,)),
    "rectangular": lambda: an.PoolNet(pool=nn.AvgPool2d((2, 3), (1, 2), (1, 1))),
    "global_pool_too": lambda: an.GlobalPoolNet(),
}


@pytest.mark.parametrize("tag", sorted(NETS))
def test_modules_with_the_avgpool_plan(nat, tag):
    from common.quantity import resident
    net, x = NETS[tag]().cuda().eval(), an.example().cuda()
    with torch.no_grad():
        plain = net(x)
    assert all(float(p.abs().max()) > 0 for p in _tuple(plain))
    off = resident.enable(net, x, concat=True)                                 # without the argument: the pool is foreign code
    plans = resident.describe(net)
    assert "resident_avgpools" not in off and "pool" not in plans and all(plans[n].emit_f32 for n in net.sources), plans
    _check_forwards(net, x, plain)

    on = resident.enable(net, x, concat=True, avgpool=True)                    # verify=True
    plans = resident.describe(net)
    assert on["resident_avgpools"] == 1 and on["fp32_outputs"] == off["fp32_outputs"] - 1, (off, on)
    assert all(not plans[n].emit_f32 for n in net.sources) and not plans["pool"].emit_f32 and plans["pool"].emit_int
    assert isinstance(net.pool.__dict__["forward"], resident._AvgPoolWindowResident)
    assert plans["pool"].relu == (tag == "relu_behind")
    if tag == "global_pool_too":
        assert isinstance(net.gpool.__dict__["forward"], resident._AvgPoolResident) and on["resident_pools"] == 1
    _check_forwards(net, x, plain)
    resident.disable(net)
    assert not resident.describe(net) and all("forward" not in m.__dict__ for m in net.modules())
    _check_forwards(net, x, plain)


@pytest.mark.parametrize("tag", ["two_bits", "add_sum_as_source", "window_9x9", "ceil_mode"])
def test_declined_plans_keep_the_fp32_form(nat, tag):
    from common.quantity import resident
    make = {"two_bits": lambda: an.PoolNet(read_bits=(4, 3)), "add_sum_as_source": lambda: an.PoolNet(mode="add_source"),
            "window_9x9": lambda: an.PoolNet(pool=nn.AvgPool2d(9, 1, 4)), "ceil_mode": lambda: an.PoolNet(pool=nn.AvgPool2d(2, ceil_mode=True))}[tag]
    net, x = make().cuda().eval(), an.example().cuda()
    with torch.no_grad():
        plain = net(x)
    on = resident.enable(net, x, concat=True, avgpool=True)
    plans = resident.describe(net)
    assert on["resident_avgpools"] == 0 and "pool" not in plans and "forward" not in net.pool.__dict__, (on, plans)
    assert plans["add" if tag == "add_sum_as_source" else "stem"].emit_f32
    _check_forwards(net, x, plain)


# ---------------------------------------------------------------- 4. golden G15 and calibrated models end to end
def test_g15_logits_equal_the_reference_with_the_switch_on(nat, oracle, golden_dir):
    """The reference's ReconModel logits of avgpool_nets.g15_net (CPU, fixed input) against the integer-simulation model on the HIP
    kernels: plain, with the parent's plan and with avgpool=True, bit for bit.  The tables come from the oracle-backed CPU
    calibration, which tests/test_avgpool_plan_cpu.py pins to the reference's byte for byte."""
    from engine_doubles import OracleCollector, OracleQuantizer
    from common.quantity import resident
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer

    with open(os.path.join(golden_dir, "g15_avgpool_net.json")) as fh:
        ref = json.load(fh)
    want = np.load(os.path.join(golden_dir, "g15_avgpool_net.npz"))["logits_recon"]
    shape = an.G15_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="cpu", max_cali_img_num=2) as tmp:
        q = CpuQuantity(cases.seed_model(an.g15_net(), base_seed=an.G15_SEED).eval())
        q.activation_quantize(cases.calib_batches(3, shape, seed=an.G15_CALIB_SEED))
        q.weight_quantize()
        q.rewrite_weight()
        wd = os.path.join(tmp, "test", "workdir")
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(cases.seed_model(an.g15_net(), base_seed=an.G15_SEED).eval())
        net = rec.ReconModel(rec.get_quantity_information(), os.path.join(wd, "recon.pth")).cuda()
        x = cases.fixed_input(shape, seed=an.G15_INPUT_SEED).cuda()
        with torch.no_grad():
            np.testing.assert_array_equal(net(x).cpu().numpy(), want)
            off = resident.enable(net, x, concat=True)
            np.testing.assert_array_equal(net(x).cpu().numpy(), want)
            on = resident.enable(net, x, concat=True, avgpool=True)
            np.testing.assert_array_equal(net(x).cpu().numpy(), want)
            np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), want[:1])
        assert on["resident_avgpools"] == 2 and off["fp32_outputs"] - on["fp32_outputs"] == 2, (off, on)


@pytest.mark.parametrize("size", [32, 64])
def test_calibrated_inception_with_the_avgpool_plan(nat, size, tmp_path):
    from common.quantity import resident
    from tools import Quantity, Reconstruction
    shape = (4, 3, size, size)
    with product_workdir(input_shape="1,3,%d,%d" % (size, size), device="gpu", max_cali_img_num=1) as tmp:
        wd = os.path.join(tmp, "test", "workdir")
        q = Quantity(an.inception(size).cuda())
        q.activation_quantize(cases.calib_batches(2, shape))
        q.weight_quantize()
        rec = Reconstruction(an.inception(size))
        net = rec.ReconModel(rec.get_quantity_information(), os.path.join(wd, "recon_avg.pth")).cuda()
        x = cases.fixed_input(shape).cuda()
        with torch.no_grad():
            plain = net(x)
        assert float(plain.std()) > 0
        off = resident.enable(net, x, concat=True)
        with torch.no_grad():
            off_out = net(x)
        on = resident.enable(net, x, concat=True, avgpool=True)                # verify=True
        plans = resident.describe(net)
        print("inception %d: off %s; on %s" % (size, off, on))
        # every pool whose source the Concat plan keeps as int8 and whose reader sits within 8 bits of it is taken
        assert on["resident_avgpools"] >= 1 and on["fp32_outputs"] < off["fp32_outputs"]
        assert on["resident_concats"] == off["resident_concats"] and on["resident_convs"] == off["resident_convs"]
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


# ---------------------------------------------------------------- 5. HIP-graph capture of the plan
def test_hipgraph_capture_of_an_avgpool_plan_replays_another_input(nat):
    """A replay on a DIFFERENT input must give that input's logits."""
    from common.quantity import resident
    for make in (an.InceptionBlockNet, lambda: an.PoolNet(relu_behind=True)):
        net = make().cuda().eval()
        x, x2 = an.example(seed=1).cuda(), an.example(seed=2).cuda() * 1.5
        with torch.no_grad():
            want, want2 = tuple(t.clone() for t in _tuple(net(x))), tuple(t.clone() for t in _tuple(net(x2)))
        assert not _same(want, want2)
        summary = resident.enable(net, x, concat=True, avgpool=True)
        assert summary["resident_avgpools"] == 1
        graphed = resident.capture(net, x)
        assert _same(graphed(x), want)
        assert _same(graphed(x2), want2)
        assert _same(graphed(x), want)
        with torch.no_grad():
            assert _same(net(x2), want2)


# ---------------------------------------------------------------- 6. the model at the benchmark's plane
def test_inception_224_32_images_on_equals_off_equals_plain(nat):
    """Synthetic bits (no calibration): output bits from one float forward's abs-max, the four branch ends of a block on the
    smallest of their bits, input bit = the producer's output bit (avgpool_nets.inception_info): all five pools are taken."""
    from common.quantity import resident
    float_model = an.inception(224, classes=100)
    x = cases.fixed_input((32, 3, 224, 224)).cuda()
    bits = dn.measured_out_bits(copy.deepcopy(float_model).cuda(), x[:8])
    net = dn.rebuild(float_model, an.inception_info(float_model, bits)).cuda()
    with torch.no_grad():
        plain = net(x)
    assert float(plain.std(dim=0).max()) > 0                                   # the images are told apart
    off = resident.enable(net, x, verify=False, concat=True)
    with torch.no_grad():
        assert torch.equal(net(x), plain)
    on = resident.enable(net, x, verify=False, concat=True, avgpool=True)
    print("inception 224: off %s; on %s" % (off, on))
    assert on["resident_avgpools"] == 5 and on["resident_concats"] == 12 and on["fp32_outputs"] == off["fp32_outputs"] - 5
    with torch.no_grad():
        assert torch.equal(net(x), plain)
