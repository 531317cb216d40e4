"""Atrous depthwise int8 convolution (fq_dwconv2d_dil_i8_resident and its _pcs / _act forms, csrc/fq_dwconv_dil_i8.hip) against
the exact integer oracle, what it declines, the NewConv2d switch `use_atrous_i8`, and resident.enable(..., depthwise=True) on
model/deeplab/DeepLabV3Plus_fabu.py.  Everything is integers: every comparison is exact.   pytest -m gpu"""
import copy
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import yaml
from torch import nn

import atrous_cases
import per_channel_chain as pcc
from test_gpu_depthwise_i8 import _dev, _expected_q, _make_case, _pad16
from workdir_util import product_workdir

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


def _run(nat, x, w, b, pad, d, rs, ob, relu, **kw):
    """One launch through the wrapper: (int8 NHWC result on the host, the variant log)."""
    nat.conv_variant_log = {}
    try:
        got = nat.dwconv2d_dil_i8_resident(x, w, b, pad, (d, d), rs, ob, relu, **kw).cpu().numpy()
        return got, dict(nat.conv_variant_log)
    finally:
        nat.conv_variant_log = None


# ---------------------------------------------------------------- 1. the kernel against the oracle
@pytest.mark.parametrize("case", atrous_cases.KERNEL_CASES, ids=atrous_cases.case_id)
def test_atrous_kernel_vs_integer_oracle(nat, oracle, case):
    R, d, ph, pw, C, H, W, N, rs, relu = case
    rng = np.random.default_rng(1000 * R + 100 * d + 10 * ph + C + H)
    xq, wq, qb, x_nhwc = _make_case(rng, R, 1, 0, C, H, W, N)
    acc = oracle.conv2d_int(xq, wq, (1, 1), (ph, pw), (d, d), groups=C)
    ob = 4 if relu else 0
    got, log = _run(nat, _dev(x_nhwc), nat.pack_weight_dw(_dev(wq.astype(np.float32))), _dev(qb), (ph, pw), d, rs, ob, relu)
    assert log == {"depthwise_dilated": 1}, log
    assert got.shape == (N, H + 2 * ph - d * (R - 1), W + 2 * pw - d * (R - 1), _pad16(C))
    np.testing.assert_array_equal(got[..., :C], _expected_q(oracle, acc, qb, rs, ob, relu))
    assert not got[..., C:].any()                                  # garbage in the input's padding channels does not come out


# ---------------------------------------------------------------- 2. the other forms
@pytest.mark.parametrize("form", ["pcs", "act", "constant_vector"])
@pytest.mark.parametrize("R,d,pad,C,H,W,N", [(3, 4, 4, 19, 9, 13, 3), (5, 2, 8, 100, 6, 9, 1)])
def test_per_channel_shift_clip_and_constant_vector_forms(nat, oracle, form, R, d, pad, C, H, W, N):
    rng = np.random.default_rng(77 + C + R)
    xq, wq, qb, x_nhwc = _make_case(rng, R, 1, 0, C, H, W, N)
    acc = oracle.conv2d_int(xq, wq, (1, 1), (pad, pad), (d, d), groups=C)
    x, w, b = _dev(x_nhwc), nat.pack_weight_dw(_dev(wq.astype(np.float32))), _dev(qb)
    if form == "pcs":                                              # one shift per channel against the per-channel oracle
        rs_k = rng.integers(1, 17, size=C).astype(np.int32)
        rs_k[0], rs_k[-1] = 16, 1
        for relu in (False, True):
            got, log = _run(nat, x, w, b, (pad, pad), d, nat.ShiftVec(_dev(rs_k), int(rs_k.min()), int(rs_k.max())), 3, relu)
            assert log == {"depthwise_dilated": 1}
            np.testing.assert_array_equal(got[..., :C], _expected_q(oracle, acc, qb, rs_k, 3, relu))
            assert not got[..., C:].any()
    elif form == "act":                                            # the ReLU6 clip of output bit 2: the Sp range [0, 24]
        clip = nat.relu6_clip(2)
        assert clip == (0, 24)
        got, log = _run(nat, x, w, b, (pad, pad), d, 7, 2, True, clip=clip)
        assert log == {"depthwise_dilated": 1}
        want = _expected_q(oracle, acc, qb, 7, 2, False)           # (a clamp of the Sp clamp is the clamp to the inner range)
        np.testing.assert_array_equal(got[..., :C], np.clip(want, 0, 24))
        assert not got[..., C:].any() and (want > 24).any() and (want < 0).any()
    else:                                                          # a constant vector: the bytes of the per-tensor entry point
        for rs in (1, 9, 16):
            sv = nat.ShiftVec(_dev(np.full(C, rs, np.int32)), rs, rs)
            a, _ = _run(nat, x, w, b, (pad, pad), d, sv, 2, True)
            c, _ = _run(nat, x, w, b, (pad, pad), d, rs, 2, True)
            np.testing.assert_array_equal(a, c)


# ---------------------------------------------------------------- 3. what the kernel declines
FQ_ERR_UNSUPPORTED = -4
#            C, R, S, sh, sw, ph, pw, dh, dw, rs
DECLINED = {"dilation 1": (32, 3, 3, 1, 1, 1, 1, 1, 1, 7), "stride 2": (32, 3, 3, 2, 2, 2, 2, 2, 2, 7),
            "dil_h != dil_w": (32, 3, 3, 1, 1, 2, 2, 2, 3, 7), "7x7": (32, 7, 7, 1, 1, 6, 6, 2, 2, 7),
            "padding beyond the span": (32, 3, 3, 1, 1, 5, 4, 2, 2, 7), "shift 17": (32, 3, 3, 1, 1, 2, 2, 2, 2, 17)}


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_cases_launch_nothing(nat, name):
    C, R, S, sh, sw, ph, pw, dh, dw, rs = DECLINED[name]
    L = nat.lib()
    assert L.fq_dwconv2d_dil_i8_supported(32, 3, 3, 1, 1, 2, 2, 7, 7) == 1
    if name != "padding beyond the span":                          # (the padding is the entry point's to judge)
        assert L.fq_dwconv2d_dil_i8_supported(C, R, S, sh, sw, dh, dw, rs, rs) == 0
    x = torch.zeros(1, 20, 20, 32, dtype=torch.int8, device="cuda")
    w = torch.zeros(7, 7, 32, dtype=torch.int8, device="cuda")
    b = torch.zeros(32, device="cuda")
    q = torch.full((1, 40, 40, 32), 5, dtype=torch.int8, device="cuda")
    vp = ctypes.c_void_p
    rc = L.fq_dwconv2d_dil_i8_resident(vp(x.data_ptr()), vp(w.data_ptr()), vp(b.data_ptr()), vp(q.data_ptr()), 32, 0, 1, 20, 20, C, R,
                                       S, sh, sw, ph, pw, dh, dw, rs, 0, None)
    torch.cuda.synchronize()
    assert rc == FQ_ERR_UNSUPPORTED and bool((q == 5).all())      # the sentinel stays


# ---------------------------------------------------------------- 4. NewConv2d with the switch, and the plan on DeepLabV3+
@pytest.mark.parametrize("C,k,d,pd,H,W,listed", [(19, 3, 2, 2, 9, 11, False), (32, 5, 3, 6, 12, 7, True), (100, 3, 12, 12, 7, 7, True)])
def test_newconv2d_switch_equals_the_default_forward(nat, C, k, d, pd, H, W, listed):
    from common.quantity import NewConv2d
    torch.manual_seed(C + k)
    conv = nn.Conv2d(C, C, k, padding=pd, dilation=d, groups=C)
    with torch.no_grad():
        conv.weight.mul_(torch.rand(C, 1, 1, 1) * 3 + 0.05)            # channel ranges that differ, as after merge_bn
    wb0, tb = pcc.numpy_channel_bits(conv.weight.detach().numpy())
    info = {"weight_bit": [min(b, 12) for b in wb0] if listed else min(tb, 12), "bias_bit": 4, "input_bit": 4, "output_bit": 4}
    x = (torch.randn(3, C, H, W) * 3).cuda()
    off, on = NewConv2d(copy.deepcopy(conv).cuda(), info), NewConv2d(copy.deepcopy(conv).cuda(), info)
    on.use_atrous_i8 = True
    assert on._atrous_ok(on.Conv) and not off._atrous_ok(off.Conv) and not on._depthwise_ok(on.Conv, True)
    nat.conv_variant_log = {}
    try:
        with torch.no_grad():
            y_off = off(x)
            assert nat.conv_variant_log == {}                          # the reference-shaped form: no integer kernel
            y_on = on(x)
        assert nat.conv_variant_log == {"depthwise_dilated": 1}
    finally:
        nat.conv_variant_log = None
    assert y_on.dtype == torch.float32 and torch.equal(y_on, y_off) and float(y_on.abs().max()) > 0
    np.testing.assert_array_equal(y_on.cpu().numpy(), pcc.ChainLayer(conv, info)(x.cpu()).numpy())


SWITCHES = dict(depthwise=True, relu6=True, concat=True, flatten=True, bilinear=True, requant=True)


@pytest.mark.parametrize("output_stride", [16, 8])
def test_deeplab_planned_with_the_attribute_on_keeps_its_logits(nat, output_stride, monkeypatch):
    """DeepLabV3Plus(width_mult 0.25, 64 x 64), calibrated on two batches: with use_atrous_i8 on, every depthwise layer is a
    resident one, fewer tensors leave the integers than with it off, and the logits are the plain forward's bit for bit."""
    from common.quantity import NewConv2d, merge_bn, resident
    from model.deeplab.DeepLabV3Plus_fabu import DeepLabV3Plus
    import cases
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("recon_fuzz", os.path.join(root, "scripts", "recon_fuzz.py"))
    rf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rf)

    def mk():
        model = DeepLabV3Plus(num_classes=5, output_stride=output_stride, width_mult=0.25, input_size=64)
        return merge_bn(cases.seed_model(model).eval()).cuda()

    data = [(b.cuda(), None) for b, _ in cases.calib_batches(2, (4, 3, 64, 64))]
    out = sys.stdout
    try:
        with product_workdir(input_shape="1,3,64,64", device="gpu", max_cali_img_num=1) as tmp:
            # SUPPORT_DILATION: the weights are quantised as they are (the default unrolls dilation 2 into a dense 5x5, the
            # reference's form for a target without dilation, and knows no other rate)
            path = os.path.join(tmp, "tools", "configs.yml")
            with open(path) as fh:
                cfg = yaml.safe_load(fh)
            cfg["SETTINGS"]["SUPPORT_DILATION"] = True
            with open(path, "w") as fh:
                yaml.safe_dump(cfg, fh)
            net = rf.recon_of(mk(), mk(), data).cuda()
    finally:
        sys.stdout = out
    x = cases.fixed_input((4, 3, 64, 64)).cuda()
    dws = [m for m in net.modules() if isinstance(m, NewConv2d) and m.Conv.groups > 1]
    dilated = [m for m in dws if m.Conv.dilation[0] > 1]
    assert len(dws) == 20 and len(dilated) == (4 if output_stride == 16 else 11) + 3
    with torch.no_grad():
        plain = net(x).clone()
        off = resident.enable(net, x, **SWITCHES)
        assert torch.equal(net(x), plain)
        monkeypatch.setattr(NewConv2d, "use_atrous_i8", True)
        assert [m._atrous_left(m.Conv) for m in dilated] == [None] * len(dilated)
        on = resident.enable(net, x, **SWITCHES)
        nat.conv_variant_log = {}
        try:
            got = net(x).clone()
            log = dict(nat.conv_variant_log)
        finally:
            nat.conv_variant_log = None
    print("DeepLabV3+ output stride %d: off %s\n on %s" % (output_stride, off, on))
    assert tuple(plain.shape) == (4, 5, 64, 64) and float(plain.std()) > 0
    assert torch.equal(got, plain)
    assert log.get("depthwise_dilated") == len(dilated) and log.get("depthwise") == len(dws) - len(dilated), log
    assert off["resident_depthwise"] == len(dws) - len(dilated) and on["resident_depthwise"] == len(dws)
    assert on["fp32_outputs"] < off["fp32_outputs"]
