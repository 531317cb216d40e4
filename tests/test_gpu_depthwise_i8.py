"""Depthwise int8 convolution (fq_dwconv2d_i8_resident / _pcs, csrc/fq_dwconv_i8.hip) against the exact integer oracle, the
NewConv2d switch `use_depthwise_i8`, and resident.enable(..., depthwise=True) on separable networks.  Everything is integers:
every comparison is exact.   pytest -m gpu"""
import ctypes
import itertools

import numpy as np
import pytest
import torch
from torch import nn

import per_channel_chain as pcc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pad16(c):
    return (c + 15) // 16 * 16


# ---------------------------------------------------------------- 1. the kernel against the oracle
def _kernel_cases():
    """{3x3, 5x5} x {stride 1, 2} x padding {0, R//2, R-1}, two cases per geometry; over them every C of {1, 16, 19, 32, 100, 256},
    odd H != W from images smaller than a lane's tile (4 output columns, 4 / 2 output rows) up to 112 x 112, N in {1, 3},
    rs in {1, 7, 16}, ob in {0, 4}, ReLU on / off."""
    chans = itertools.cycle([1, 16, 19, 32, 100, 256, 19])         # (period 7 against the 6 cases of a kernel size x stride)
    small = itertools.cycle([(5, 7), (7, 5), (9, 13), (6, 11), (5, 6), (17, 9)])
    big = itertools.cycle([(33, 29), (57, 55), (29, 41), (112, 112)])
    shifts = itertools.cycle([1, 7, 16])
    cases = []
    i = 0
    for R in (3, 5):
        for st in (1, 2):
            for pd in (0, R // 2, R - 1):
                for size in (small, big):
                    C = next(chans)
                    H, W = next(size)
                    if (H, W) == (112, 112) and C > 32:
                        C = 32                                   # (the largest plane at a width the oracle walks quickly)
                    cases.append((R, st, pd, C, H, W, 1 if (H * W * C > 100000 or i % 3 == 0) else 3, next(shifts),
                                  4 * ((i // 3) % 2), bool((i + i // 6) % 2)))
                    i += 1
    # images smaller than the kernel and than one lane's tile (they exist only behind padding)
    cases += [(3, 1, 1, 19, 1, 2, 3, 7, 0, True), (3, 2, 2, 16, 2, 1, 1, 1, 4, False), (5, 1, 2, 100, 2, 3, 3, 16, 4, True),
              (5, 2, 4, 1, 1, 1, 1, 7, 0, False), (3, 1, 1, 256, 3, 3, 1, 16, 0, False), (5, 2, 2, 32, 3, 5, 3, 1, 4, True)]
    return cases


KERNEL_CASES = _kernel_cases()


def test_the_case_list_covers_what_it_claims():
    cs = KERNEL_CASES
    assert {(c[0], c[1]) for c in cs} == {(3, 1), (3, 2), (5, 1), (5, 2)}
    assert {(c[0], c[2]) for c in cs} >= {(R, p) for R in (3, 5) for p in (0, R // 2, R - 1)}
    assert {c[3] for c in cs} == {1, 16, 19, 32, 100, 256}
    assert {c[6] for c in cs} == {1, 3} and {c[7] for c in cs} == {1, 7, 16} and {c[8] for c in cs} == {0, 4}
    assert {c[9] for c in cs} == {True, False} and any((c[4], c[5]) == (112, 112) for c in cs)
    assert all(c[4] != c[5] or (c[4], c[5]) in ((112, 112), (1, 1), (3, 3)) for c in cs)


def _make_case(rng, R, st, pd, C, H, W, N):
    xq = rng.integers(-128, 128, size=(N, C, H, W)).astype(np.int32)
    wq = rng.integers(-128, 128, size=(C, 1, R, R)).astype(np.int32)
    xq.flat[::11] = -128
    wq.flat[::7] = -128                                            # (-128) * (-128) products in every sum
    qb = rng.integers(-128, 128, size=C).astype(np.float32)
    qb[::5] = np.resize([300.0, -1e5, 3e9, -40000.0, 255.0, -256.0], len(qb[::5]))      # beyond the output range: saturation
    cpad = _pad16(C)
    x_nhwc = rng.integers(-128, 128, size=(N, H, W, cpad)).astype(np.int8)            # padding channels hold garbage
    x_nhwc[..., :C] = xq.transpose(0, 2, 3, 1)
    return xq, wq, qb, x_nhwc


def _expected_q(oracle, acc, qb, rs, ob, relu):
    """acc int32 [N, C, P, Q] -> int8 NHWC (real channels): the reference's fp32 tail, ReLU, the next layer's Quantity(ob)."""
    if np.ndim(rs) == 0:
        y = oracle.recon_epilogue(acc.astype(np.float32), qb, int(rs), ob)
    else:
        y = pcc.pc_epilogue(acc.astype(np.float32), qb, rs, ob)
    if relu:
        y = np.maximum(y, np.float32(0))
    return oracle.quantity(y, ob).astype(np.int8).transpose(0, 2, 3, 1)


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "r%d_s%d_p%d_c%d_%dx%d_n%d_rs%d_ob%d_relu%d" % c)
def test_dwconv_kernel_vs_integer_oracle(nat, oracle, case):
    R, st, pd, C, H, W, N, rs, ob, relu = case
    rng = np.random.default_rng(1000 * R + 100 * st + 10 * pd + C + H)
    xq, wq, qb, x_nhwc = _make_case(rng, R, st, pd, C, H, W, N)
    acc = oracle.conv2d_int(xq, wq, (st, st), (pd, pd), (1, 1), groups=C)
    w_dev = nat.pack_weight_dw(_dev(wq.astype(np.float32)))
    assert tuple(w_dev.shape) == (R, R, _pad16(C)) and not w_dev[..., C:].any()
    nat.conv_variant_log = {}
    try:
        got = nat.dwconv2d_i8_resident(_dev(x_nhwc), w_dev, _dev(qb), (st, st), (pd, pd), rs, ob, relu).cpu().numpy()
        log = dict(nat.conv_variant_log)
    finally:
        nat.conv_variant_log = None
    assert log == {"depthwise": 1}, log
    assert got.shape == (N,) + acc.shape[2:] + (_pad16(C),)
    np.testing.assert_array_equal(got[..., :C], _expected_q(oracle, acc, qb, rs, ob, relu))
    assert not got[..., C:].any()                                  # garbage in the input's padding channels does not come out


# ---------------------------------------------------------------- 2. one shift per channel
@pytest.mark.parametrize("R,st,pd,C,H,W,N", [(3, 1, 1, 19, 9, 13, 3), (3, 2, 0, 100, 15, 11, 1), (5, 1, 2, 32, 7, 9, 2),
                                               (5, 2, 4, 256, 11, 6, 1), (3, 1, 2, 1, 5, 4, 3)])
def test_dwconv_pcs_vs_per_channel_oracle_and_constant_vector(nat, oracle, R, st, pd, C, H, W, N):
    rng = np.random.default_rng(77 + C + R)
    xq, wq, qb, x_nhwc = _make_case(rng, R, st, pd, C, H, W, N)
    acc = oracle.conv2d_int(xq, wq, (st, st), (pd, pd), (1, 1), groups=C)
    w_dev, x_dev, b_dev = nat.pack_weight_dw(_dev(wq.astype(np.float32))), _dev(x_nhwc), _dev(qb)
    rs_k = rng.integers(1, 17, size=C).astype(np.int32)
    rs_k[0], rs_k[-1] = 16, 1
    for relu in (False, True):
        sv = nat.ShiftVec(_dev(rs_k), int(rs_k.min()), int(rs_k.max()))
        nat.conv_variant_log = {}
        try:
            got = nat.dwconv2d_i8_resident(x_dev, w_dev, b_dev, (st, st), (pd, pd), sv, 3, relu).cpu().numpy()
            assert nat.conv_variant_log == {"depthwise": 1}
        finally:
            nat.conv_variant_log = None
        np.testing.assert_array_equal(got[..., :C], _expected_q(oracle, acc, qb, rs_k, 3, relu))
        assert not got[..., C:].any()
    for rs in (1, 9, 16):                                          # a constant vector: the bytes of the per-tensor entry point
        sv = nat.ShiftVec(_dev(np.full(C, rs, np.int32)), rs, rs)
        a = nat.dwconv2d_i8_resident(x_dev, w_dev, b_dev, (st, st), (pd, pd), sv, 2, True)
        b = nat.dwconv2d_i8_resident(x_dev, w_dev, b_dev, (st, st), (pd, pd), rs, 2, True)
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 3. what the kernel declines
FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED = -1, -4


def _raw_call(nat, x, w, b, q, cpad, C, R, S, sh, sw, ph, pw, dh, dw, rs, N=1, H=9, W=9):
    vp = ctypes.c_void_p
    return nat.lib().fq_dwconv2d_i8_resident(vp(x.data_ptr()), vp(w.data_ptr()), vp(b.data_ptr()), vp(q.data_ptr()) if q is not None else None,
                                            cpad, 0, N, H, W, C, R, S, sh, sw, ph, pw, dh, dw, rs, 0, None)


def test_declined_cases_and_argument_errors(nat):
    L = nat.lib()
    ok = (32, 3, 3, 1, 1, 1, 1, 7, 7)
    assert L.fq_dwconv2d_i8_supported(*ok) == 1
    assert L.fq_dwconv2d_i8_supported(32, 5, 5, 2, 2, 1, 1, 1, 16) == 1
    declined = {
        "dilation 2": (32, 3, 3, 1, 1, 2, 2, 7, 7), "7x7": (32, 7, 7, 1, 1, 1, 1, 7, 7), "1x1": (32, 1, 1, 1, 1, 1, 1, 7, 7),
        "3x5": (32, 3, 5, 1, 1, 1, 1, 7, 7), "stride 3": (32, 3, 3, 3, 3, 1, 1, 7, 7), "stride 1x2": (32, 3, 3, 1, 2, 1, 1, 7, 7),
        "rs 0": (32, 3, 3, 1, 1, 1, 1, 0, 0), "rs 17": (32, 3, 3, 1, 1, 1, 1, 17, 17), "rs 0..7": (32, 3, 3, 1, 1, 1, 1, 0, 7),
        "rs 7..17": (32, 3, 3, 1, 1, 1, 1, 7, 17),
    }
    x = torch.zeros(1, 9, 9, 32, dtype=torch.int8, device="cuda")
    w = torch.zeros(7, 7, 32, dtype=torch.int8, device="cuda")
    b = torch.zeros(32, device="cuda")
    q = torch.full((1, 9, 9, 32), 5, dtype=torch.int8, device="cuda")
    for name, (C, R, S, sh, sw, dh, dw, lo, hi) in declined.items():
        assert L.fq_dwconv2d_i8_supported(C, R, S, sh, sw, dh, dw, lo, hi) == 0, name
        if lo == hi:
            assert _raw_call(nat, x, w, b, q, 32, C, R, S, sh, sw, 1, 1, dh, dw, lo) == FQ_ERR_UNSUPPORTED, name
    assert _raw_call(nat, x, w, b, q, 32, 32, 3, 3, 1, 1, 3, 3, 1, 1, 7) == FQ_ERR_UNSUPPORTED        # padding >= R
    # as the other integer entry points: channels not padded to 16 -> unsupported, no output pointer -> invalid argument
    assert _raw_call(nat, x, w, b, q, 24, 24, 3, 3, 1, 1, 1, 1, 1, 1, 7) == FQ_ERR_UNSUPPORTED
    assert _raw_call(nat, x, w, b, None, 32, 32, 3, 3, 1, 1, 1, 1, 1, 1, 7) == FQ_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((q == 5).all())                                    # nothing was launched
    assert _raw_call(nat, x, w, b, q, 32, 32, 3, 3, 1, 1, 1, 1, 1, 1, 7) == 0
    torch.cuda.synchronize()
    assert bool((q == 0).all())


# ---------------------------------------------------------------- 4. NewConv2d with the switch
import copy                                                           # noqa: E402

import cases                                                          # noqa: E402
import depthwise_nets as dn                                           # noqa: E402
from workdir_util import product_workdir                              # noqa: E402

LAYER_CASES = [(16, 3, 1, 1, 9, 11), (19, 3, 2, 1, 12, 7), (100, 5, 1, 2, 7, 7), (32, 5, 2, 2, 10, 13), (64, 3, 1, 0, 6, 5)]


@pytest.mark.parametrize("C,k,st,pd,H,W", LAYER_CASES)
@pytest.mark.parametrize("listed", [False, True], ids=["per_tensor", "per_channel"])
def test_newconv2d_switch_equals_the_default_forward_and_the_cpu_chain(nat, C, k, st, pd, H, W, listed):
    from common.quantity import NewConv2d
    torch.manual_seed(C + k)
    conv = nn.Conv2d(C, C, k, stride=st, padding=pd, groups=C)
    with torch.no_grad():
        conv.weight.mul_(torch.rand(C, 1, 1, 1) * 3 + 0.05)            # channel ranges that differ, as after merge_bn
    wb0, tb = pcc.numpy_channel_bits(conv.weight.detach().numpy())
    info = {"weight_bit": [min(b, 12) for b in wb0] if listed else min(tb, 12), "bias_bit": 4, "input_bit": 4, "output_bit": 4}
    if listed:
        assert len(set(info["weight_bit"])) > 1
    x = torch.randn(3, C, H, W) * 3
    want = pcc.ChainLayer(conv, info)(x)
    off = NewConv2d(copy.deepcopy(conv).cuda(), info)
    on = NewConv2d(copy.deepcopy(conv).cuda(), info)
    on.use_depthwise_i8 = True
    assert on._depthwise_ok(on.Conv) and not off._depthwise_ok(off.Conv) and not on._int8_ok(on.Conv)
    nat.conv_variant_log = {}
    try:
        with torch.no_grad():
            y_off = off(x.cuda())
            assert nat.conv_variant_log == {}                              # the reference-shaped form: no integer kernel
            y_on = on(x.cuda())
        assert nat.conv_variant_log == {"depthwise": 1}
    finally:
        nat.conv_variant_log = None
    assert isinstance(y_on, torch.Tensor) and y_on.dtype == torch.float32 and y_on.shape == y_off.shape
    assert torch.equal(y_on, y_off)
    np.testing.assert_array_equal(y_on.cpu().numpy(), want.numpy())
    assert float(y_on.abs().max()) > 0


# ---------------------------------------------------------------- 5. calibrated networks end to end
def _mobilenet(residual, size):
    from model.mobilenet.MobileNet_fabu import MobileNet
    return lambda: MobileNet(num_classes=10, input_size=size, residual=residual)


E2E_MODELS = {"tiny": (cases.tiny_separable_net, 16), "v1_32": (_mobilenet(False, 32), 32), "v1_64": (_mobilenet(False, 64), 64),
              "res_32": (_mobilenet(True, 32), 32), "res_64": (_mobilenet(True, 64), 64)}


def _dw_layers(net):
    from common.quantity import NewConv2d
    return [(n, m) for n, m in net.named_modules() if isinstance(m, NewConv2d) and m.Conv.groups > 1]


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("tag", sorted(E2E_MODELS))
def test_calibrated_separable_models_with_the_depthwise_plan(nat, tag, per_channel, monkeypatch):
    from common.quantity import merge_bn, resident
    from tools import Quantity, Reconstruction
    fn, size = E2E_MODELS[tag]
    shape = (4, 3, size, size)
    float_model = merge_bn(cases.seed_model(fn()).eval())
    if tag == "tiny":
        monkeypatch.setattr(torch, "save", lambda *a, **k: None)       # the fixture net is a local class: not picklable
    with product_workdir(input_shape="1,3,%d,%d" % (size, size), device="gpu", max_cali_img_num=1) as tmp:
        import os
        wd = os.path.join(tmp, "test", "workdir")
        q = Quantity(copy.deepcopy(float_model).cuda())
        q.activation_quantize(cases.calib_batches(2, shape))
        q.weight_quantize()
        if per_channel:
            q.weight_quantize_per_channel()
        rec = Reconstruction(copy.deepcopy(float_model))
        info = rec.get_quantity_information_per_channel() if per_channel else rec.get_quantity_information()
        net = rec.ReconModel(info, os.path.join(wd, "recon_dw.pth")).cuda()
        x = cases.fixed_input(shape).cuda()
        with torch.no_grad():
            plain = net(x)
            ref = pcc.cpu_chain(float_model, info)(x.cpu())
        np.testing.assert_array_equal(plain.cpu().numpy(), ref.numpy())
        assert float(plain.std()) > 0

        dws = _dw_layers(net)
        assert len(dws) == (3 if tag == "tiny" else 13)
        resident.enable(net, x)                                            # the default: grouped convolutions stay fp32 producers
        plans = resident.describe(net)
        assert all(n not in plans or (plans[n].emit_f32 and not plans[n].depthwise) for n, _ in dws)
        with torch.no_grad():
            assert torch.equal(net(x), plain)

        summary = resident.enable(net, x, depthwise=True)                  # verify=True
        plans = resident.describe(net)
        taken = [n for n, m in dws if 1 <= (m.rs_min if isinstance(m.rs_bit, list) else m.rs_bit)
                 and (m.rs_max if isinstance(m.rs_bit, list) else m.rs_bit) <= 16]
        declined = [n for n, _ in dws if n not in taken]
        print("%s %s: depthwise layers taken %d, declined for their shift: %s" % (tag, "pc" if per_channel else "pt", len(taken), declined))
        assert len(taken) >= 2, declined
        assert summary["resident_depthwise"] == len(taken)
        for n in taken:
            assert plans[n].depthwise and plans[n].emit_int, (n, plans[n])
        for n in declined:
            assert n not in plans or not plans[n].depthwise
        nat.conv_variant_log = {}
        try:
            with torch.no_grad():
                got = net(x)
            assert nat.conv_variant_log.get("depthwise", 0) == len(taken), nat.conv_variant_log
        finally:
            nat.conv_variant_log = None
        assert torch.equal(got, plain)
        np.testing.assert_array_equal(got.cpu().numpy(), ref.numpy())
        with torch.no_grad():
            assert torch.equal(net(x[:1]), plain[:1])
            assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
        resident.disable(net)
        with torch.no_grad():
            assert torch.equal(net(x), plain)


# ---------------------------------------------------------------- 6. HIP-graph capture of the plan
def test_hipgraph_capture_of_a_depthwise_plan_replays_another_input(nat):
    """As test_gpu_resident.py does for a non-stem first layer: a replay on a DIFFERENT input must give that input's logits."""
    from common.quantity import resident
    for make, shape in ((lambda: dn.seeded(cases.tiny_separable_net().eval()), (4, 3, 16, 16)),
                        (lambda: dn.seeded(dn.SeparableAddNet().eval(), seed=5), (4, 3, 8, 8))):
        model = make()
        net = dn.rebuild(model, dn.fixed_info(model, per_channel=True)).cuda()
        x, x2 = cases.fixed_input(shape, seed=1).cuda(), cases.fixed_input(shape, seed=2).cuda() * 2
        with torch.no_grad():
            want, want2 = net(x).clone(), net(x2).clone()
        assert not torch.equal(want, want2)
        summary = resident.enable(net, x, depthwise=True)
        assert summary["resident_depthwise"] >= 2
        graphed = resident.capture(net, x)
        assert torch.equal(graphed(x), want)
        assert torch.equal(graphed(x2), want2)
        assert torch.equal(graphed(x), want)
        with torch.no_grad():
            assert torch.equal(net(x2), want2)


# ---------------------------------------------------------------- 7. the model at the benchmark's size
@pytest.mark.parametrize("residual", [False, True], ids=["v1", "residual"])
def test_mobilenet_224_256_images_on_equals_off_equals_plain(nat, residual):
    """Synthetic bits (no calibration): output bits from one float forward's abs-max, weight bits per channel from the folded
    weights, input bit = the producer's output bit."""
    from common.quantity import merge_bn, resident
    from model.mobilenet.MobileNet_fabu import MobileNet
    float_model = merge_bn(cases.seed_model(MobileNet(num_classes=100, input_size=224, residual=residual)).eval())
    x = cases.fixed_input((256, 3, 224, 224)).cuda()
    bits = dn.measured_out_bits(copy.deepcopy(float_model).cuda(), x[:8])
    info = dn.fixed_info(float_model, per_channel=True, image_bit=5, out_bit_of=bits)
    net = dn.rebuild(float_model, info).cuda()
    with torch.no_grad():
        plain = net(x)
    assert float(plain.std(dim=0).max()) > 0                               # the images are told apart
    off = resident.enable(net, x, verify=False)
    with torch.no_grad():
        assert torch.equal(net(x), plain)
    on = resident.enable(net, x, verify=False, depthwise=True)
    takeable = [n for n, m in _dw_layers(net) if 1 <= m.rs_min and m.rs_max <= 16]
    print("mobilenet 224 residual=%s: %d of 13 depthwise layers taken; off %s; on %s" % (residual, len(takeable), off, on))
    assert on["resident_depthwise"] == len(takeable) >= 10
    assert on["resident_convs"] == off["resident_convs"] + len(takeable)
    nat.conv_variant_log = {}
    try:
        with torch.no_grad():
            got = net(x)
        assert nat.conv_variant_log.get("depthwise", 0) == len(takeable)
    finally:
        nat.conv_variant_log = None
    assert torch.equal(got, plain)
