"""The `_act` entry points of the integer producers (fq_conv2d_i8_resident_act, fq_conv2d_i8_stem_act, fq_dwconv2d_i8_resident_act,
fq_gconv2d_i8_resident_act and their per-channel-shift forms) with the Sp range of a fused nn.ReLU6, against the exact oracle
expectation: the reference's fp32 tail (recon_epilogue) -> torch.nn.functional.relu6 -> the next layer's Quantity(ob).  Everything
is integers: every comparison is exact.   pytest -m gpu"""
import numpy as np
import pytest
import torch

import per_channel_chain as pcc

pytestmark = pytest.mark.gpu

OBS = (-1, 0, 2, 4, 5)
SHIFTS = (1, 7, 16)
# kind -> (C, K, groups, kernel, stride, pad, H, W, N): the smallest shapes that still reach every code path
SHAPES = {
    "dense1x1": (16, 24, 1, 1, 1, 0, 5, 7, 3),
    "dense3x3s2": (16, 32, 1, 3, 2, 1, 9, 13, 2),
    "stem": (3, 16, 1, 3, 2, 1, 32, 32, 2),
    "dw19s1": (19, 19, 19, 3, 1, 1, 6, 11, 2),
    "dw19s2": (19, 19, 19, 3, 2, 1, 6, 11, 2),
    "dw32s1": (32, 32, 32, 3, 1, 1, 6, 11, 2),
    "dw32s2": (32, 32, 32, 3, 2, 1, 6, 11, 2),
    "grouped": (32, 32, 4, 3, 1, 1, 6, 11, 2),
}
STEM_IB = 3


@pytest.fixture(scope="module")
def nat():
    from common.quantity import _native
    _native.lib()
    return _native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pad16(c):
    return (c + 15) // 16 * 16


def _data(kind, rs, bound, seed):
    """Integer operands whose outputs land on both sides of the clip: full-range inputs with (-128) * (-128) products, the LAST
    image all zeros (its outputs are the bias alone), weights scaled to the shift so that the shifted accumulator has a spread of
    a few units, and biases that cycle through the inside of (0, bound), the bound itself, just beyond it, negative values and
    values far beyond the output range on both sides (the ones tail_consts clamps)."""
    C, K, G, R, st, pd, H, W, N = SHAPES[kind]
    rng = np.random.default_rng(seed)
    x = rng.integers(-128, 128, size=(N, C, H, W)).astype(np.int32)
    x.flat[::11] = -128
    x[-1] = 0
    taps = (C // G) * R * R
    amp = int(min(127, max(1, round(2.0 ** rs * 4 / (taps ** 0.5 * 74)))))
    w = rng.integers(-amp, amp + 1, size=(K, C // G, R, R)).astype(np.int32)
    if amp == 127:
        w.flat[::7] = -128
    inside = max(1, bound // 2)
    # (3e9 is beyond int32.  The stem kernel adds its bias as an int32, fq_stem.hip -- the six-instruction tail, no tail_consts
    #  clamp -- so its largest bias here is 2e9: still far beyond the output range, and r + qb stays inside int32)
    huge = 2e9 if kind == "stem" else 3e9
    qb = np.resize(np.array([inside, bound, 1, -1, bound + 5, 300.0, -1e5, 0, huge, bound - 1, -40000.0, -129, 127, 255.0, -256.0, 2],
                            dtype=np.float32), K)
    return x, w, qb


def _acc(oracle, kind, x, w):
    C, K, G, R, st, pd, H, W, N = SHAPES[kind]
    return oracle.conv2d_int(x, w, (st, st), (pd, pd), (1, 1), groups=G) if G > 1 else oracle.conv2d_int(x, w, (st, st), (pd, pd), (1, 1))


def _expected(oracle, acc, qb, rs, ob):
    """acc int32 [N, K, P, Q] -> (fp32 NCHW behind the ReLU6, int8 NHWC the next layer's Quantity(ob) reads)."""
    if np.ndim(rs) == 0:
        y = oracle.recon_epilogue(acc.astype(np.float32), qb, int(rs), ob)
    else:
        y = pcc.pc_epilogue(acc.astype(np.float32), qb, rs, ob)
    y = torch.nn.functional.relu6(torch.from_numpy(y)).numpy()
    return y, oracle.quantity(y, ob).astype(np.int8).transpose(0, 2, 3, 1)


def _launch(nat, kind, x, w, qb, rs, ob, clip, want_f32=False):
    """(fp32 NCHW or None, int8 NHWC) of the producer `kind` with relu=True and the Sp range `clip`."""
    C, K, G, R, st, pd, H, W, N = SHAPES[kind]
    wf, b = _dev(w.astype(np.float32)), _dev(qb)
    if kind == "stem":
        xf = _dev(x.astype(np.float32) * np.float32(2.0 ** -STEM_IB))            # Quantity(STEM_IB) recovers x exactly
        return None, nat.conv2d_i8_stem(xf, nat.pack_weight_stem(wf), b, K, R, (st, st), (pd, pd), STEM_IB, rs, ob, True, clip=clip)
    cpad = _pad16(C)
    xq = np.random.default_rng(5).integers(-128, 128, size=(N, H, W, cpad)).astype(np.int8)     # garbage in the padding channels
    if G == 1:
        xq[..., C:] = 0                                                          # (the dense kernels read them: zero by contract)
    xq[..., :C] = x.transpose(0, 2, 3, 1)
    if G == C:
        return None, nat.dwconv2d_i8_resident(_dev(xq), nat.pack_weight_dw(wf), b, (st, st), (pd, pd), rs, ob, True, clip=clip)
    if G > 1:
        return None, nat.gconv2d_i8_resident(_dev(xq), nat.pack_weight_grouped(wf, G), b, K, G, (st, st), (pd, pd), rs, ob, True,
                                             clip=clip)
    return nat.conv2d_i8_resident(_dev(xq), nat.pack_weight_krsc(wf), b, (st, st), (pd, pd), (1, 1), rs, ob, want_f32, True, True,
                                  clip=clip)


@pytest.mark.parametrize("ob", OBS)
@pytest.mark.parametrize("kind", sorted(SHAPES))
def test_act_entry_points_vs_the_oracle_chain_with_relu6(nat, oracle, kind, ob):
    C, K, G, R, st, pd, H, W, N = SHAPES[kind]
    clip = nat.relu6_clip(ob)
    bound = clip[1]
    assert clip == (0, min(127, int(6 * 2.0 ** ob)))
    for rs in SHIFTS:
        x, w, qb = _data(kind, rs, bound, 100 * (ob + 1) + rs + len(kind))
        acc = _acc(oracle, kind, x, w)
        want_y, want_q = _expected(oracle, acc, qb, rs, ob)
        assert (want_q == bound).any() and ((want_q > 0) & (want_q < bound)).any() and (want_q == 0).any(), (kind, ob, rs)
        assert int(want_q.max()) == bound and int(want_q.min()) == 0
        y, q = _launch(nat, kind, x, w, qb, rs, ob, clip, want_f32=True)
        q = q.cpu().numpy()
        assert q.shape == want_q.shape[:3] + (_pad16(K),)
        np.testing.assert_array_equal(q[..., :K], want_q, err_msg="%s ob %d rs %d" % (kind, ob, rs))
        assert not q[..., K:].any()
        if y is not None:                                                        # the dense entry point's fp32 output, clipped too
            np.testing.assert_array_equal(y.cpu().numpy(), want_y)
        # one shift per channel: the _pcs_act form; a constant vector gives the per-tensor bytes
        sv = nat.ShiftVec(_dev(np.full(K, rs, np.int32)), rs, rs)
        _y, qc = _launch(nat, kind, x, w, qb, sv, ob, clip)
        assert torch.equal(qc.cpu(), torch.from_numpy(q))
    rng = np.random.default_rng(7 + ob)
    rs_k = rng.integers(1, 17, size=K).astype(np.int32)
    rs_k[0], rs_k[-1] = 16, 1
    x, w, qb = _data(kind, 7, bound, 901 + ob + len(kind))
    acc = _acc(oracle, kind, x, w)
    _want_y, want_q = _expected(oracle, acc, qb, rs_k, ob)
    assert (want_q == bound).any() and ((want_q > 0) & (want_q < bound)).any()
    _y, q = _launch(nat, kind, x, w, qb, nat.ShiftVec(_dev(rs_k), 1, 16), ob, clip)
    np.testing.assert_array_equal(q.cpu().numpy()[..., :K], want_q)


def test_the_range_of_a_plain_relu_gives_the_plain_entry_points_bytes(nat, oracle):
    """(0, 127) and (-128, 127) through `_act` are relu = 1 and relu = 0 of the entry points without it."""
    for kind in sorted(SHAPES):
        x, w, qb = _data(kind, 7, 96, 3)
        for relu, clip in ((True, (0, 127)), (False, (-128, 127))):
            _y, a = _launch(nat, kind, x, w, qb, 7, 4, clip)
            C, K, G, R, st, pd, H, W, N = SHAPES[kind]
            acc = _acc(oracle, kind, x, w)
            y = oracle.recon_epilogue(acc.astype(np.float32), qb, 7, 4)
            if relu:
                y = np.maximum(y, np.float32(0))
            np.testing.assert_array_equal(a.cpu().numpy()[..., :K], oracle.quantity(y, 4).astype(np.int8).transpose(0, 2, 3, 1))


def test_a_range_outside_the_contract_is_refused(nat):
    x, w, qb = _data("dw19s1", 7, 96, 1)
    for clip in ((1, 96), (0, 128), (-129, 5)):
        with pytest.raises(nat.FqError):
            _launch(nat, "dw19s1", x, w, qb, 7, 4, clip)
