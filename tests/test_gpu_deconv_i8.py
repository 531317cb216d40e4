"""fq_deconv2d_i8_resident on the MI355X against the float64 rule: torch's CPU conv_transpose2d in float64 on the same integers,
then the oracle's RightShift + BiasAdd + Sp (deconv_nets.f64_acc / oracle_tail), and against include/fq.h's rule written out in
numpy.  Every comparison is exact.   pytest -m gpu

The shapes (deconv_nets.kernel_cases) are the smallest at which each mechanism can go wrong: one and three images; planes 1x1,
2x3, 5x4, 8x8; C in {1, 3, 16, 17, 40} and K in {1, 5, 16, 33, 64} in pairs (one and three channel chunks, one and two
accumulators, a channel block that ends inside Kpad); kernel == stride, kernel > stride with padding and output_padding, stride 1,
kernel < stride (phases without a tap), 5 / 3 with uneven phases; a rectangular kernel with strides (2, 1); an odd chunk count;
shifts 1, 7, 16; ReLU on and off; two `_act` ranges.  Operands run over the full int8 range, -128 included, some biases saturate
both ways, the source's padding channels hold garbage, the output is pre-filled with 0x55 inside an arena whose guard bytes must
survive, and the output's padding channels are asserted zero.  One launch has more items than the capped grid has workgroups."""
import ctypes

import numpy as np
import pytest
import torch

import deconv_nets as dn

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID, UNSUPPORTED = -1, -4


def _run(c, seed, rule=True):
    from common.quantity import _native
    x, w, qb = dn.operands(np.random.default_rng(seed), c)
    acc = dn.f64_acc(x, w, c)
    want = dn.oracle_tail(acc, qb, c)
    if rule:
        np.testing.assert_array_equal(dn.rule_acc(x, w, c), acc.astype(np.int64), err_msg=dn.case_id(c))
    np.testing.assert_array_equal(dn.int_tail(acc.astype(np.int64), qb, c), want, err_msg=dn.case_id(c))
    assert _native.deconv_supported(c["C"], c["K"], 1, c["kernel"][0], c["kernel"][1], c["stride"], c["pad"], c["outpad"], (1, 1), c["rs"])
    wq = _native.pack_weight_deconv(torch.from_numpy(w.astype(np.float32)).cuda(), c["stride"], c["pad"])
    np.testing.assert_array_equal(wq.cpu().numpy(), dn.pack_rule(w, c))
    nbytes = want.size
    arena = torch.full((GUARD + nbytes + GUARD,), 0x55, dtype=torch.int8, device="cuda")
    out = arena[GUARD:GUARD + nbytes].view(want.shape)
    xd = torch.from_numpy(x).cuda()
    got = _native.deconv2d_i8_resident(xd, wq, torch.from_numpy(qb).cuda(), c["C"], c["kernel"], c["stride"], c["pad"], c["outpad"],
                                       c["rs"], 3, bool(c["relu"]), clip=c["clip"], out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = arena.cpu().numpy()
    assert (host[:GUARD] == 0x55).all() and (host[GUARD + nbytes:] == 0x55).all(), dn.case_id(c)
    res = host[GUARD:GUARD + nbytes].reshape(want.shape)
    np.testing.assert_array_equal(res, want, err_msg=dn.case_id(c))
    assert not res[..., c["K"]:].any()
    np.testing.assert_array_equal(xd.cpu().numpy(), x)                                  # the source is only read
    return want


def test_the_cases_cover_what_the_docstring_says():
    cases = dn.kernel_cases()
    assert {(c["kernel"][0], c["stride"][0], c["pad"][0], c["outpad"][0]) for c in cases if c["kernel"][0] == c["kernel"][1]
            and c["stride"][0] == c["stride"][1]} >= set(dn.KSPO)
    assert {c["N"] for c in cases} == {1, 3} and {(c["H"], c["W"]) for c in cases} >= set(dn.PLANES)
    assert {c["C"] for c in cases} == {1, 3, 16, 17, 40} and {c["K"] for c in cases} == {1, 5, 16, 33, 64}
    assert {c["rs"] for c in cases} == {1, 7, 16} and {c["relu"] for c in cases} == {0, 1} and any(c["clip"] for c in cases)
    assert any(c["kernel"] == (2, 3) and c["stride"] == (2, 1) for c in cases)
    assert dn.items(dn.BIG_CASE) > dn.MAX_BLOCKS and all(dn.items(c) <= dn.MAX_BLOCKS for c in cases)


def test_kernel_matches_the_float64_rule_and_writes_nothing_outside_its_output():
    sat_lo = sat_hi = False
    for k, c in enumerate(dn.kernel_cases()):
        want = _run(c, seed=100 + k)
        real = want[..., :c["K"]]
        lo, hi = c["clip"] if c["clip"] else ((0, 127) if c["relu"] else (-128, 127))
        sat_lo, sat_hi = sat_lo or bool((real == lo).any()), sat_hi or bool((real == hi).any())
    assert sat_lo and sat_hi


def test_a_launch_whose_workgroups_take_a_second_item():
    _run(dn.BIG_CASE, seed=7, rule=False)


def test_a_fresh_output_tensor_and_an_empty_batch():
    from common.quantity import _native
    c = dn.case(3, 5, 4, 17, 33, (3, 3), (2, 2), (1, 1), (1, 1), rs=7, relu=1)
    x, w, qb = dn.operands(np.random.default_rng(3), c)
    want = dn.oracle_tail(dn.f64_acc(x, w, c), qb, c)
    wq = _native.pack_weight_deconv(torch.from_numpy(w.astype(np.float32)).cuda(), c["stride"], c["pad"])
    xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(qb).cuda()
    got = _native.deconv2d_i8_resident(xd, wq, qd, 17, (3, 3), (2, 2), (1, 1), (1, 1), 7, 0, True)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert _native.deconv2d_i8_resident(xd[:0], wq, qd, 17, (3, 3), (2, 2), (1, 1), (1, 1), 7, 0, True).shape == (0, 10, 8, 48)
    assert _native.CONV_VARIANTS[_native.lib().fq_conv2d_i8_last_variant() & 0xff] in ("deconv", "none")


def test_every_refusal_by_return_code_with_nothing_written():
    from common.quantity import _native
    L = _native.lib()
    x = torch.full((4096,), 0x33, dtype=torch.int8, device="cuda")
    w = torch.full((4096,), 0x11, dtype=torch.int8, device="cuda")
    b = torch.zeros(8, dtype=torch.float32, device="cuda")
    y = torch.full((65536,), 0x55, dtype=torch.int8, device="cuda")
    px, pw, pb, py = (ctypes.c_void_p(t.data_ptr()) for t in (x, w, b, y))
    #       x   w   qb  q  Cpad Kpad relu N  H  W  C  K  R  S sh sw ph pw oh ow rs ob
    good = (px, pw, pb, py, 16, 16, 0, 1, 2, 2, 8, 8, 2, 2, 2, 2, 0, 0, 0, 0, 7, 0)

    def put(i, v, base=good):
        return base[:i] + (v,) + base[i + 1:]

    rows = {
        "null x": (put(0, None), INVALID), "null w": (put(1, None), INVALID), "null qbias": (put(2, None), INVALID),
        "null q": (put(3, None), INVALID), "misaligned x": (put(0, ctypes.c_void_p(px.value + 4)), INVALID),
        "misaligned w": (put(1, ctypes.c_void_p(pw.value + 8)), INVALID), "misaligned q": (put(3, ctypes.c_void_p(py.value + 4)), INVALID),
        "Cpad": (put(4, 32), INVALID), "Kpad": (put(5, 32), INVALID), "N < 0": (put(7, -1), INVALID), "H < 1": (put(8, 0), INVALID),
        "W < 1": (put(9, 0), INVALID), "C < 1": (put(10, 0), INVALID), "K < 1": (put(11, 0), INVALID), "R < 1": (put(12, 0), INVALID),
        "stride 0": (put(14, 0), INVALID), "pad < 0": (put(16, -1), INVALID), "outpad < 0": (put(19, -1), INVALID),
        "rs 121": (put(20, 121), INVALID), "ob 121": (put(21, 121), INVALID),
        "kernel 9": (put(12, 9), UNSUPPORTED), "S = 9": (put(13, 9), UNSUPPORTED), "stride 5": (put(15, 5), UNSUPPORTED),
        "pad == kernel": (put(16, 2), UNSUPPORTED), "outpad == stride": (put(18, 2), UNSUPPORTED), "rs 0": (put(20, 0), UNSUPPORTED),
        "rs 17": (put(20, 17), UNSUPPORTED), "rs -3": (put(20, -3), UNSUPPORTED),
        "an input of 2^31 bytes": (put(7, 1 << 25, put(8, 2, put(9, 2))), UNSUPPORTED),
        "N H W past 2^31": (put(8, 1 << 20, put(9, 1 << 20)), UNSUPPORTED),
        "an accumulator past int32": ((px, pw, pb, py, 8128, 16, 0, 1, 1, 1, 8128, 8, 8, 8, 2, 2, 0, 0, 0, 0, 16, 0), UNSUPPORTED),
        "a wrong scalar beats a null pointer": ((None, None, None, None) + put(12, 9)[4:], UNSUPPORTED),
    }
    f = L.fq_deconv2d_i8_resident
    for what, (a, code) in rows.items():
        assert f(*a, None) == code, what
    assert f(*((None, None, None, None) + put(7, 0)[4:]), None) == 0                         # N == 0: FQ_OK without a launch
    g = L.fq_deconv2d_i8_resident_act
    act = good[:6] + (-5, 100) + good[7:]
    for lo, hi in ((1, 100), (-129, 100), (-5, 128), (-5, -1)):
        assert g(*(act[:6] + (lo, hi) + act[8:]), None) == INVALID
    assert g(*((None, None, None, None) + act[4:13] + (9,) + act[14:]), None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == 0x55).all()) and bool((x == 0x33).all()) and bool((w == 0x11).all())
    t = torch.zeros(1, 2, 2, 16, dtype=torch.int8, device="cuda")
    wq = torch.zeros(16 * 4 * 16, dtype=torch.int8, device="cuda")
    for bad in ((t, wq, b, 8, (2, 2), (5, 5), (0, 0), (0, 0), 7, 0, False), (t, wq, b, 8, (2, 2), (2, 2), (0, 0), (0, 0), 0, 0, False),
                (t.cpu(), wq, b, 8, (2, 2), (2, 2), (0, 0), (0, 0), 7, 0, False), (t, wq[:-16], b, 8, (2, 2), (2, 2), (0, 0), (0, 0), 7, 0, False)):
        with pytest.raises((_native.FqError, AssertionError)):
            _native.deconv2d_i8_resident(*bad)
