"""Grouped int8 convolution (fq_gconv2d_i8_resident / _pcs, csrc/fq_gconv_i8.hip) against the exact integer oracle, the
NewConv2d switch `use_grouped_i8`, and resident.enable(..., grouped=True) on ResNeXt-style networks.  Everything is integers:
every comparison is exact.   pytest -m gpu"""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import cases
import depthwise_nets as dn
import grouped_doubles as gd
import grouped_nets as gn
import per_channel_chain as pcc
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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
def _make_case(rng, G, cgi, cgo, R, N, H, W):
    C, K = G * cgi, G * cgo
    xq = rng.integers(-128, 128, size=(N, C, H, W)).astype(np.int32)
    wq = rng.integers(-128, 128, size=(K, cgi, R, R)).astype(np.int32)
    xq.flat[::11] = -128
    wq.flat[::7] = -128                                            # (-128) * (-128) products in every sum
    qb = rng.integers(-128, 128, size=K).astype(np.float32)
    qb[::5] = np.resize([300.0, -1e5, 3e9, -40000.0, 255.0, -256.0], len(qb[::5]))      # beyond the output range: saturation
    x_nhwc = rng.integers(-128, 128, size=(N, H, W, _pad16(C))).astype(np.int8)        # padding channels hold garbage
    x_nhwc[..., :C] = xq.transpose(0, 2, 3, 1)
    return xq, wq, qb, x_nhwc


def _expected_q(oracle, acc, qb, rs, ob, relu):
    """acc int32 [N, K, P, Q] -> int8 NHWC (real channels): the reference's fp32 tail, ReLU, the next layer's Quantity(ob)."""
    if np.ndim(rs) == 0:
        y = oracle.recon_epilogue(acc.astype(np.float32), qb, int(rs), ob)
    else:
        y = pcc.pc_epilogue(acc.astype(np.float32), qb, rs, ob)
    if relu:
        y = np.maximum(y, np.float32(0))
    return oracle.quantity(y, ob).astype(np.int8).transpose(0, 2, 3, 1)


def _settings(i):
    """shift, ReLU and output grid of the i-th shape of a width: every shift with and without the ReLU within six shapes"""
    return (1, 7, 16)[i % 3], 4 * ((i // 6) % 2), bool((i // 3) % 2)


def test_the_settings_cycle_covers_every_shift_with_and_without_relu():
    seen = {(_settings(i)[0], _settings(i)[2]) for i in range(6)}
    assert seen == {(rs, relu) for rs in (1, 7, 16) for relu in (False, True)}
    assert {_settings(i)[1] for i in range(12)} == {0, 4}


def _run_shape(nat, oracle, shape, i):
    G, cgi, cgo, R, st, pd, N, H, W = shape
    C, K = G * cgi, G * cgo
    rs, ob, relu = _settings(i)
    rng = np.random.default_rng(sum(v * 31 ** k for k, v in enumerate(shape)) % (1 << 31))
    xq, wq, qb, x_nhwc = _make_case(rng, G, cgi, cgo, R, N, H, W)
    w_dev = nat.pack_weight_grouped(_dev(wq.astype(np.float32)), G)
    assert tuple(w_dev.shape) == (_pad16(K) // 4, R * R, cgi // 4, 4, 4) and not w_dev[K // 4:].any()
    assert torch.equal(w_dev.cpu(), gd.pack_weight_grouped(torch.from_numpy(wq.astype(np.float32)), G))
    if H + 2 * pd < R or W + 2 * pd < R:                           # the kernel does not fit: an argument error, nothing launched
        with pytest.raises(nat.FqError):
            nat.gconv2d_i8_resident(_dev(x_nhwc), w_dev, _dev(qb), K, G, (st, st), (pd, pd), rs, ob, relu)
        return 0
    acc = oracle.conv2d_int(xq, wq, (st, st), (pd, pd), (1, 1), groups=G)
    nat.conv_variant_log = {}
    try:
        got = nat.gconv2d_i8_resident(_dev(x_nhwc), w_dev, _dev(qb), K, G, (st, st), (pd, pd), rs, ob, relu).cpu().numpy()
        log = dict(nat.conv_variant_log)
    finally:
        nat.conv_variant_log = None
    assert log == {"grouped": 1}, (shape, log)
    assert got.shape == (N,) + acc.shape[2:] + (_pad16(K),), shape
    np.testing.assert_array_equal(got[..., :K], _expected_q(oracle, acc, qb, rs, ob, relu), err_msg=str(shape))
    assert not got[..., K:].any(), shape                           # output padding channels are zero
    return 1


@pytest.mark.parametrize("width", gd.GROUP_WIDTHS, ids=lambda w: "g%d_cgi%d_cgo%d" % w)
def test_gconv_kernel_vs_integer_oracle(nat, oracle, width):
    shapes = [s for s in gd.kernel_shapes() if s[:3] == width and s != gd.MANY_TILES]
    assert len(shapes) == (2 + 6) * len(gd.PLANES) * len(gd.BATCHES)
    ran = sum(_run_shape(nat, oracle, s, i) for i, s in enumerate(shapes))
    assert ran >= 60                                               # (the planes a 3x3 does not fit without padding are the rest)


def test_gconv_kernel_with_more_tiles_than_workgroups(nat, oracle):
    G, cgi, cgo, R, st, pd, N, H, W = gd.MANY_TILES
    assert N * H * ((W + 3) // 4) * (G * cgo // 64) > 2048 * (256 // 16)       # strip blocks x channel blocks > workgroups
    assert _run_shape(nat, oracle, gd.MANY_TILES, 7) == 1


# ---------------------------------------------------------------- 2. one shift per channel; the output as a view
@pytest.mark.parametrize("G,cgi,cgo,R,st,pd,N,H,W", [(3, 8, 4, 3, 1, 1, 3, 9, 11), (5, 4, 12, 1, 2, 0, 1, 5, 7),
                                                      (2, 64, 64, 3, 2, 2, 2, 7, 9), (32, 4, 4, 3, 1, 0, 1, 6, 5),
                                                      (2, 16, 8, 1, 1, 0, 3, 2, 2)])
def test_gconv_pcs_vs_per_channel_oracle_and_constant_vector(nat, oracle, G, cgi, cgo, R, st, pd, N, H, W):
    K = G * cgo
    rng = np.random.default_rng(77 + K + R)
    xq, wq, qb, x_nhwc = _make_case(rng, G, cgi, cgo, R, N, H, W)
    acc = oracle.conv2d_int(xq, wq, (st, st), (pd, pd), (1, 1), groups=G)
    w_dev, x_dev, b_dev = nat.pack_weight_grouped(_dev(wq.astype(np.float32)), G), _dev(x_nhwc), _dev(qb)
    rs_k = rng.integers(1, 17, size=K).astype(np.int32)
    rs_k[0], rs_k[-1] = 16, 1
    for relu in (False, True):
        sv = nat.ShiftVec(_dev(rs_k), int(rs_k.min()), int(rs_k.max()))
        nat.conv_variant_log = {}
        try:
            got = nat.gconv2d_i8_resident(x_dev, w_dev, b_dev, K, G, (st, st), (pd, pd), sv, 3, relu).cpu().numpy()
            assert nat.conv_variant_log == {"grouped": 1}
        finally:
            nat.conv_variant_log = None
        np.testing.assert_array_equal(got[..., :K], _expected_q(oracle, acc, qb, rs_k, 3, relu))
        assert not got[..., K:].any()
    for rs in (1, 9, 16):                                          # a constant vector: the bytes of the per-tensor entry point
        sv = nat.ShiftVec(_dev(np.full(K, rs, np.int32)), rs, rs)
        a = nat.gconv2d_i8_resident(x_dev, w_dev, b_dev, K, G, (st, st), (pd, pd), sv, 2, True)
        b = nat.gconv2d_i8_resident(x_dev, w_dev, b_dev, K, G, (st, st), (pd, pd), rs, 2, True)
        assert torch.equal(a, b)


FQ_ERR_INVALID_ARG, FQ_ERR_UNSUPPORTED = -1, -4


def _raw(nat, x, w, b, q, C, K, G, R=3, S=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, rs=7, N=1, H=9, W=9, cpad=None, kpad=None,
         relu=0):
    vp = ctypes.c_void_p

    def ptr(t):
        return None if t is None else vp(t if isinstance(t, int) else t.data_ptr())
    return nat.lib().fq_gconv2d_i8_resident(ptr(x), ptr(w), ptr(b), ptr(q), _pad16(C) if cpad is None else cpad,
                                           _pad16(K) if kpad is None else kpad, relu, N, H, W, C, K, G, R, S, sh, sw, ph, pw, dh,
                                           dw, rs, 0, None)


@pytest.mark.parametrize("G,cgi,cgo,R,st,pd,N,H,W", [(3, 8, 4, 3, 1, 1, 3, 5, 7), (5, 4, 12, 1, 1, 0, 1, 9, 11),
                                                      (8, 4, 4, 3, 2, 0, 3, 33, 17)])
def test_the_output_is_written_between_its_sentinels_and_nowhere_else(nat, oracle, G, cgi, cgo, R, st, pd, N, H, W):
    C, K = G * cgi, G * cgo
    rng = np.random.default_rng(5 + K)
    xq, wq, qb, x_nhwc = _make_case(rng, G, cgi, cgo, R, N, H, W)
    acc = oracle.conv2d_int(xq, wq, (st, st), (pd, pd), (1, 1), groups=G)
    P, Q = acc.shape[2:]
    n = N * P * Q * _pad16(K)
    buf = torch.full((n + 512,), 0x5a, dtype=torch.int8, device="cuda")
    off = 256 + (-buf.data_ptr()) % 16                              # a 16-byte aligned view with sentinels on both sides
    x_dev, w_dev, b_dev = _dev(x_nhwc), nat.pack_weight_grouped(_dev(wq.astype(np.float32)), G), _dev(qb)
    rc = _raw(nat, x_dev, w_dev, b_dev, buf.data_ptr() + off, C, K, G, R, R, st, st, pd, pd, N=N, H=H, W=W, relu=1)
    assert rc == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:off] == 0x5a).all() and (host[off + n:] == 0x5a).all()
    got = host[off:off + n].reshape(N, P, Q, _pad16(K))
    np.testing.assert_array_equal(got[..., :K], _expected_q(oracle, acc, qb, 7, 0, True))
    assert not got[..., K:].any()


# ---------------------------------------------------------------- 3. what the kernel declines
def test_declined_cases_and_argument_errors(nat):
    L = nat.lib()
    assert L.fq_gconv2d_i8_supported(32, 32, 8, 3, 3, 1, 1, 1, 1, 7, 7) == 1
    assert L.fq_gconv2d_i8_supported(128, 128, 2, 1, 1, 2, 2, 1, 1, 1, 16) == 1
    # (C, K, G, R, S, sh, sw, dh, dw, lo, hi)
    declined = {
        "dense": (32, 32, 1, 3, 3, 1, 1, 1, 1, 7, 7), "depthwise": (32, 32, 32, 3, 3, 1, 1, 1, 1, 7, 7),
        "cgi 2": (32, 64, 16, 3, 3, 1, 1, 1, 1, 7, 7), "cgi 6": (24, 16, 4, 3, 3, 1, 1, 1, 1, 7, 7),
        "cgi 68": (136, 16, 2, 3, 3, 1, 1, 1, 1, 7, 7), "cgo 3": (32, 24, 8, 3, 3, 1, 1, 1, 1, 7, 7),
        "cgo 68": (16, 136, 2, 3, 3, 1, 1, 1, 1, 7, 7), "5x5": (32, 32, 8, 5, 5, 1, 1, 1, 1, 7, 7),
        "3x1": (32, 32, 8, 3, 1, 1, 1, 1, 1, 7, 7), "dilation 2": (32, 32, 8, 3, 3, 1, 1, 2, 2, 7, 7),
        "stride 3": (32, 32, 8, 3, 3, 3, 3, 1, 1, 7, 7), "stride 1x2": (32, 32, 8, 3, 3, 1, 2, 1, 1, 7, 7),
        "rs 0": (32, 32, 8, 3, 3, 1, 1, 1, 1, 0, 0), "rs 17": (32, 32, 8, 3, 3, 1, 1, 1, 1, 17, 17),
        "rs 0..7": (32, 32, 8, 3, 3, 1, 1, 1, 1, 0, 7), "rs 7..17": (32, 32, 8, 3, 3, 1, 1, 1, 1, 7, 17),
    }
    x = torch.zeros(1, 9, 9, 144, dtype=torch.int8, device="cuda")
    w = torch.zeros(144 * 25 * 68, dtype=torch.int8, device="cuda")
    b = torch.zeros(144, device="cuda")
    q = torch.full((1, 9, 9, 144), 5, dtype=torch.int8, device="cuda")
    for name, (C, K, G, R, S, sh, sw, dh, dw, lo, hi) in declined.items():
        assert L.fq_gconv2d_i8_supported(C, K, G, R, S, sh, sw, dh, dw, lo, hi) == 0, name
        if lo == hi:
            assert _raw(nat, x, w, b, q, C, K, G, R, S, sh, sw, 0, 0, dh, dw, lo) == FQ_ERR_UNSUPPORTED, name
    assert _raw(nat, x, w, b, q, 32, 32, 8, ph=3, pw=3) == FQ_ERR_UNSUPPORTED                      # padding >= R
    assert _raw(nat, x, w, b, q, 32, 32, 8, 1, 1, ph=1, pw=1) == FQ_ERR_UNSUPPORTED
    assert _raw(nat, x, w, b, q, 64, 64, 2, N=1 << 12, H=1 << 8, W=1 << 8) == FQ_ERR_UNSUPPORTED   # 32-bit offsets
    invalid = {
        "no output": dict(q=None), "no input": dict(x=None), "no weights": dict(w=None), "no bias": dict(b=None),
        "misaligned output": dict(q=q.data_ptr() + 4), "misaligned input": dict(x=x.data_ptr() + 8),
        "misaligned weights": dict(w=w.data_ptr() + 1), "H 0": dict(H=0), "N -1": dict(N=-1), "groups 0": dict(G=0),
        "stride 0": dict(sh=0, sw=0), "pad -1": dict(ph=-1), "Cpad 48": dict(cpad=48), "Kpad 24": dict(kpad=24),
        "Cpad 16": dict(cpad=16), "C % groups": dict(C=36, K=32, G=8), "K % groups": dict(C=32, K=36, G=8),
        "plane below the kernel": dict(H=1, W=1, ph=0, pw=0),
    }
    for name, kw in invalid.items():
        args = dict(x=x, w=w, b=b, q=q, C=32, K=32, G=8)
        args.update(kw)
        assert _raw(nat, **args) == FQ_ERR_INVALID_ARG, name
    assert _raw(nat, None, None, None, None, 32, 32, 8, N=0) == 0                                  # an empty batch is fine
    torch.cuda.synchronize()
    assert bool((q == 5).all())                                    # nothing was launched
    assert _raw(nat, x, w, b, q, 32, 32, 8) == 0
    torch.cuda.synchronize()
    assert bool((q.view(-1)[:9 * 9 * 32] == 0).all()) and bool((q.view(-1)[9 * 9 * 32:] == 5).all())


# ---------------------------------------------------------------- 4. NewConv2d with the switch
LAYER_CASES = [(2, 4, 4, 3, 1, 1, 9, 11), (3, 8, 4, 3, 2, 1, 12, 7), (5, 4, 12, 1, 1, 0, 7, 7), (2, 64, 64, 3, 2, 2, 10, 13),
               (32, 4, 4, 3, 1, 0, 6, 5), (2, 16, 8, 1, 2, 0, 5, 9)]


@pytest.mark.parametrize("G,cgi,cgo,k,st,pd,H,W", LAYER_CASES)
@pytest.mark.parametrize("listed", [False, True], ids=["per_tensor", "per_channel"])
def test_newconv2d_switch_equals_the_default_forward_and_the_cpu_chain(nat, G, cgi, cgo, k, st, pd, H, W, listed):
    from common.quantity import NewConv2d
    C, K = G * cgi, G * cgo
    torch.manual_seed(C + k)
    conv = nn.Conv2d(C, K, k, stride=st, padding=pd, groups=G)
    with torch.no_grad():
        conv.weight.mul_(torch.rand(K, 1, 1, 1) * 3 + 0.05)            # channel ranges that differ, as after merge_bn
    wb0, tb = pcc.numpy_channel_bits(conv.weight.detach().numpy())
    info = {"weight_bit": [min(b, 12) for b in wb0] if listed else min(tb, 12), "bias_bit": 4, "input_bit": 4, "output_bit": 4}
    if listed:
        assert len(set(info["weight_bit"])) > 1
    x = torch.randn(3, C, H, W) * 3
    want = pcc.ChainLayer(conv, info)(x)
    off = NewConv2d(copy.deepcopy(conv).cuda(), info)
    on = NewConv2d(copy.deepcopy(conv).cuda(), info)
    on.use_grouped_i8 = True
    assert on._grouped_ok(on.Conv) and not off._grouped_ok(off.Conv) and not on._int8_ok(on.Conv)
    nat.conv_variant_log = {}
    try:
        with torch.no_grad():
            y_off = off(x.cuda())
            assert nat.conv_variant_log == {}                              # the reference-shaped form: no integer kernel
            y_on = on(x.cuda())
        assert nat.conv_variant_log == {"grouped": 1}
    finally:
        nat.conv_variant_log = None
    assert isinstance(y_on, torch.Tensor) and y_on.dtype == torch.float32 and y_on.shape == y_off.shape
    assert torch.equal(y_on, y_off)
    np.testing.assert_array_equal(y_on.cpu().numpy(), want.numpy())
    assert float(y_on.abs().max()) > 0


# ---------------------------------------------------------------- 5. the toy nets with and without the argument
TOY_NETS = {"resnext": gn.ToyResNeXt, "pointwise": gn.GroupedPointwiseNet, "mixed": gn.GroupedDepthwiseNet, "add": gn.GroupedAddNet}


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("tag", sorted(TOY_NETS))
def test_toy_nets_with_and_without_the_argument(nat, tag, per_channel):
    from common.quantity import resident
    cls = TOY_NETS[tag]
    model = gn.seeded(cls().eval())
    info = gn.fixed_info(model, per_channel=per_channel)
    net = gn.rebuild(model, info).cuda()
    x = cases.fixed_input((4, 3, 8, 8), seed=1).cuda()
    with torch.no_grad():
        plain = net(x)
        ref = pcc.cpu_chain(model, info)(x.cpu())
    np.testing.assert_array_equal(plain.cpu().numpy(), ref.numpy())
    assert float(plain.std()) > 0
    off = resident.enable(net, x)
    assert "resident_grouped" not in off and not any(p.grouped for p in resident.describe(net).values())
    with torch.no_grad():
        assert torch.equal(net(x), plain)
    on = resident.enable(net, x, grouped=True, depthwise=(tag == "mixed"))
    plans = resident.describe(net)
    assert on["resident_grouped"] == len(cls.GROUPED) and all(plans[n].grouped and not plans[n].emit_f32 for n in cls.GROUPED)
    assert on["fused_conv_adds"] >= off["fused_conv_adds"] and on["fused_block_tails"] >= off["fused_block_tails"]
    nat.conv_variant_log = {}
    try:
        with torch.no_grad():
            got = net(x)
        assert nat.conv_variant_log.get("grouped", 0) == len(cls.GROUPED), nat.conv_variant_log
        if tag == "mixed":
            assert nat.conv_variant_log.get("depthwise", 0) == 1
    finally:
        nat.conv_variant_log = None
    assert torch.equal(got, plain)
    with torch.no_grad():
        assert torch.equal(net(x[:1]), plain[:1])
        assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
    resident.disable(net)
    with torch.no_grad():
        assert torch.equal(net(x), plain)


# ---------------------------------------------------------------- 6. golden G16 and calibrated ResNeXt models end to end
def _grouped_layers(net):
    from common.quantity import NewConv2d
    return [(n, m) for n, m in net.named_modules() if isinstance(m, NewConv2d) and 1 < m.Conv.groups < m.Conv.in_channels]


def _calibrated(float_model, shape, per_channel, tmp, name):
    from tools import Quantity, Reconstruction
    wd = os.path.join(tmp, "test", "workdir")
    q = Quantity(copy.deepcopy(float_model).cuda())
    q.activation_quantize(cases.calib_batches(2, shape))
    q.weight_quantize()
    if per_channel:
        q.weight_quantize_per_channel()
    rec = Reconstruction(copy.deepcopy(float_model))
    info = rec.get_quantity_information_per_channel() if per_channel else rec.get_quantity_information()
    return rec.ReconModel(info, os.path.join(wd, name)).cuda(), info


def test_g16_logits_on_the_gpu_engine_bit_for_bit(nat):
    """The reference's ReconModel logits of golden G16 from the GPU engine's own calibration: plain, the default plan, grouped."""
    from common.quantity import resident
    with open(os.path.join(GOLDEN, "g16_grouped_net.json")) as fh:
        ref = json.load(fh)
    arrays = np.load(os.path.join(GOLDEN, "g16_grouped_net.npz"))
    from tools import Quantity, Reconstruction
    shape = gn.G16_SHAPE
    with product_workdir(input_shape="1,%d,%d,%d" % shape[1:], device="gpu", max_cali_img_num=2) as tmp:
        wd = os.path.join(tmp, "test", "workdir")
        q = Quantity(cases.seed_model(gn.g16_net(), base_seed=gn.G16_SEED).eval().cuda())
        q.activation_quantize(cases.calib_batches(3, shape, seed=gn.G16_CALIB_SEED))
        assert open(os.path.join(wd, "feat.table")).read() == ref["feat_table"]
        q.weight_quantize()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table"]
        q.rewrite_weight()
        assert open(os.path.join(wd, "weight.table")).read() == ref["weight_table_rewritten"]
        rec = Reconstruction(cases.seed_model(gn.g16_net(), base_seed=gn.G16_SEED).eval())
        net = rec.ReconModel(rec.get_quantity_information(), os.path.join(wd, "recon.pth")).cuda()
        x = torch.from_numpy(arrays["x"]).cuda()
        with torch.no_grad():
            np.testing.assert_array_equal(net(x).cpu().numpy(), arrays["logits_recon"])
            resident.enable(net, x)
            np.testing.assert_array_equal(net(x).cpu().numpy(), arrays["logits_recon"])
            on = resident.enable(net, x, grouped=True)
            assert on["resident_grouped"] == 2
            nat.conv_variant_log = {}
            try:
                np.testing.assert_array_equal(net(x).cpu().numpy(), arrays["logits_recon"])
                assert nat.conv_variant_log.get("grouped", 0) == 2
            finally:
                nat.conv_variant_log = None
            np.testing.assert_array_equal(net(x[:1]).cpu().numpy(), arrays["logits_recon"][:1])


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("size", [32, 64])
def test_calibrated_resnext_with_the_grouped_plan(nat, size, per_channel):
    import io
    from common.quantity import merge_bn, resident
    from model.resnext.ResNeXt_fabu import ResNeXt50
    shape = (4, 3, size, size)
    # BatchNorm scales of 0.35 .. 1.05 (gamma_scale): with the default 0.5 .. 1.5 the residual blocks double the activations' range
    # block after block and the calibrated logits at 64 x 64 are all zero
    float_model = merge_bn(cases.seed_model(ResNeXt50(num_classes=10, input_size=size), gamma_scale=0.7).eval())
    with product_workdir(input_shape="1,3,%d,%d" % (size, size), device="gpu", max_cali_img_num=1) as tmp:
        net, info = _calibrated(float_model, shape, per_channel, tmp, "recon_gc.pth")
        x = cases.fixed_input(shape).cuda()
        with torch.no_grad():
            plain = net(x)
            ref = pcc.cpu_chain(float_model, info)(x.cpu())
        np.testing.assert_array_equal(plain.cpu().numpy(), ref.numpy())
        assert float(plain.std()) > 0

        gcs = _grouped_layers(net)
        assert len(gcs) == 16 and sorted({m.Conv.in_channels // m.Conv.groups for _, m in gcs}) == [4, 8, 16, 32]
        off = resident.enable(net, x)                                      # the default: grouped convolutions stay fp32 producers
        plans = resident.describe(net)
        assert all(n not in plans for n, _ in gcs) and "resident_grouped" not in off
        with torch.no_grad():
            assert torch.equal(net(x), plain)

        summary = resident.enable(net, x, grouped=True)                    # verify=True
        plans = resident.describe(net)
        taken = [n for n, m in gcs if m._grouped_ok(m.Conv, True)]
        declined = [n for n, _ in gcs if n not in taken]
        print("resnext %d %s: grouped layers taken %d, declined for their shift: %s; off %s; on %s"
              % (size, "pc" if per_channel else "pt", len(taken), declined, off, summary))
        assert len(taken) >= 2, declined
        assert summary["resident_grouped"] == len(taken) and summary["resident_convs"] == off["resident_convs"] + len(taken)
        assert summary["fused_conv_adds"] >= off["fused_conv_adds"] and summary["fused_block_tails"] >= off["fused_block_tails"]
        for n in taken:
            assert plans[n].grouped and plans[n].emit_int and plans[n].relu and not plans[n].emit_f32, (n, plans[n])
            assert not plans[n.replace("conv2", "conv1")].emit_f32        # the 1x1 in front no longer writes fp32
        for n in declined:
            assert n not in plans
        nat.conv_variant_log = {}
        try:
            with torch.no_grad():
                got = net(x)
            assert nat.conv_variant_log.get("grouped", 0) == len(taken), nat.conv_variant_log
        finally:
            nat.conv_variant_log = None
        assert torch.equal(got, plain)
        with torch.no_grad():
            assert torch.equal(net(x[:1]), plain[:1])
            assert torch.equal(net(torch.flip(x, dims=[0])), torch.flip(plain, dims=[0]))
        # save / load: the plan travels with the modules, the packed weights are rebuilt
        buf = io.BytesIO()
        torch.save(net, buf)
        buf.seek(0)
        again = torch.load(buf, weights_only=False)
        assert sum(p.grouped for p in resident.describe(again).values()) == len(taken)
        assert "_w_gc" not in dict(again.named_modules())[taken[0]].__dict__
        with torch.no_grad():
            assert torch.equal(again(x), plain)
        resident.disable(net)
        assert not resident.describe(net)
        with torch.no_grad():
            assert torch.equal(net(x), plain)


# ---------------------------------------------------------------- 7. HIP-graph capture of the plan
def test_hipgraph_capture_of_a_grouped_plan_replays_another_input(nat):
    """A replay on a DIFFERENT input must give that input's logits."""
    from common.quantity import resident
    for cls in (gn.ToyResNeXt, gn.GroupedAddNet):
        model = gn.seeded(cls().eval())
        net = gn.rebuild(model, gn.fixed_info(model, per_channel=True)).cuda()
        x, x2 = cases.fixed_input((4, 3, 8, 8), seed=1).cuda(), cases.fixed_input((4, 3, 8, 8), seed=2).cuda() * 2
        with torch.no_grad():
            want, want2 = net(x).clone(), net(x2).clone()
        assert not torch.equal(want, want2)
        summary = resident.enable(net, x, grouped=True)
        assert summary["resident_grouped"] == 2
        graphed = resident.capture(net, x)
        assert torch.equal(graphed(x), want)
        assert torch.equal(graphed(x2), want2)
        assert torch.equal(graphed(x), want)
        with torch.no_grad():
            assert torch.equal(net(x2), want2)


# ---------------------------------------------------------------- 8. the model at the cost script's plane size
def test_resnext_224_16_images_on_equals_off_equals_plain(nat):
    """Synthetic bits (no calibration): output bits from one float forward's abs-max, weight bits per channel from the folded
    weights, input bit = the producer's output bit."""
    from common.quantity import merge_bn, resident
    from model.resnext.ResNeXt_fabu import ResNeXt50
    # BatchNorm scales of 0.35 .. 1.05: with seed_model's default 0.5 .. 1.5 the sixteen residual blocks double the activations'
    # range block after block, the output bits run down to -9 and the integer logits of every image are 0
    float_model = merge_bn(cases.seed_model(ResNeXt50(num_classes=100, input_size=224), gamma_scale=0.7).eval())
    x = cases.fixed_input((16, 3, 224, 224)).cuda()
    bits = dn.measured_out_bits(copy.deepcopy(float_model).cuda(), x[:4])
    info = gn.fixed_info(float_model, per_channel=True, image_bit=5, out_bit_of=bits, sources=gn.bottleneck_sources(float_model))
    net = gn.rebuild(float_model, info).cuda()
    with torch.no_grad():
        plain = net(x)
    assert float(plain.std(dim=0).max()) > 0                               # the images are told apart
    off = resident.enable(net, x, verify=False)
    with torch.no_grad():
        assert torch.equal(net(x), plain)
    on = resident.enable(net, x, verify=False, grouped=True)
    takeable = [n for n, m in _grouped_layers(net) if m._grouped_ok(m.Conv, True)]
    print("resnext 224: %d of 16 grouped layers taken; off %s; on %s" % (len(takeable), off, on))
    assert on["resident_grouped"] == len(takeable) >= 2
    assert on["resident_convs"] == off["resident_convs"] + len(takeable)
    assert on["fused_conv_adds"] >= off["fused_conv_adds"] and on["fused_block_tails"] >= off["fused_block_tails"]
    nat.conv_variant_log = {}
    try:
        with torch.no_grad():
            got = net(x)
        assert nat.conv_variant_log.get("grouped", 0) == len(takeable)
    finally:
        nat.conv_variant_log = None
    assert torch.equal(got, plain)
