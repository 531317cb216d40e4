"""tests/limit_refs.py (the torch expressions the size-limit GPU tests take their expected values from) against the CPU oracle, on
small adversarial arrays: rounding ties on both sides, saturation, biases far outside the output range, values on the edges of
histogram bins.  Every comparison is exact.  No GPU: the helpers run on CPU tensors here, the same operations as on the device."""
import numpy as np
import pytest
import torch

import limit_refs as lr
from int_conv_ref import add_resident_ref
from per_channel_chain import pc_epilogue


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _tail_operands():
    """The accumulators of test_conv_tail_rounding_ties_and_saturation (every int8 value times k - 32, some rows pushed far out of
    range) and the biases of test_a_bias_far_outside_the_output_range...: [1][64][16][16] fp32, [64] fp32."""
    K = 64
    x = np.arange(-128, 128).reshape(1, 1, 16, 16).astype(np.int64)
    acc = x * (np.arange(K) - 32).reshape(1, K, 1, 1) + 127 * np.where(np.arange(K) % 3 == 0, 127, 0).reshape(1, K, 1, 1)
    qb = ((np.arange(K) % 7) - 3).astype(np.float32)
    qb[::7] = [(-1) ** i * v for i, v in enumerate(np.resize([300.0, 1e5, 3e9, 40000.0, 255.0, 256.0], len(qb[::7])))]
    return acc.astype(np.float32), qb


@pytest.mark.parametrize("rs", [1, 2, 7, 8, 12, 16, 17, 20, 0, -2])
def test_per_tensor_tail_relu_and_the_next_quantity_equal_the_oracle(oracle, rs):
    acc, qb = _tail_operands()
    for ob in (0, 3, 4):
        ref = oracle.recon_epilogue(acc, qb, rs, ob)
        got = lr.recon_epilogue(_t(acc), _t(qb), rs, ob)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), ref), (rs, ob)
        rref = np.maximum(ref, np.float32(0))
        assert np.array_equal(lr.relu(got).numpy(), rref)
        for ib in (ob, ob - 1, ob + 2):                                    # the next layer's Quantity: same grid, coarser, finer
            assert np.array_equal(lr.quantity(lr.relu(got), ib).numpy(), oracle.quantity(rref, ib)), (rs, ob, ib)


def test_rightshift_ties_equal_the_oracle(oracle):
    """Exact halves on both sides of zero, their neighbours, and magnitudes whose fp32 sum with 0.5 rounds."""
    x = np.concatenate([np.arange(-1040, 1041), [2 ** 24, 2 ** 24 + 2, -(2 ** 24) - 2, 2 ** 31, -(2 ** 31), 3e9, -3e9, 0.0]]).astype(np.float32)
    for rs in (1, 2, 3, 5, 0, -1):
        assert np.array_equal(lr.rightshift(_t(x), rs).numpy(), oracle.rightshift(x, rs)), rs


def test_per_channel_tail_equals_the_oracle_channel_by_channel(oracle):
    acc, qb = _tail_operands()
    rs = [(3 * k) % 20 - 1 for k in range(acc.shape[1])]                   # -1 .. 18: the integer tail's range and both sides of it
    for ob in (0, 3):
        ref = pc_epilogue(acc, qb, rs, ob)
        got = lr.pc_epilogue(_t(acc), _t(qb), torch.tensor(rs, dtype=torch.int32), ob)
        assert np.array_equal(got.numpy(), ref), ob


def test_quandequan_and_add_sat_equal_the_oracle(oracle):
    x = np.concatenate([np.arange(-1100, 1101) * 0.25, [1e9, -1e9, 127.5, -128.5, 126.5]]).astype(np.float32)
    for bit in (-2, -1, 0, 1, 3):
        assert np.array_equal(lr.quandequan(_t(x), bit).numpy(), oracle.quandequan(x, bit)), bit
        assert np.array_equal(lr.quantity(_t(x), bit).numpy(), oracle.quantity(x, bit)), bit
    a = np.arange(-260, 261).astype(np.float32)
    b = a[::-1].copy() * np.float32(0.5)
    assert np.array_equal(lr.add_sat(_t(a), _t(b)).numpy(), oracle.add_sat(a, b))
    assert np.array_equal(lr.add_sat(_t(a), _t(a)).numpy(), oracle.add_sat(a, a))


def test_add_resident_equals_the_numpy_statement_of_fq_h():
    rng = np.random.default_rng(7)
    for x_dtype, gx, y_dtype, gy, ib, relu in ((np.int8, 3, np.int8, 5, 4, True), (np.int8, 3, np.int16, 6, 4, False),
                                               (np.int16, 8, np.int16, 8, 2, True), (np.int8, 0, np.int8, 0, 0, False),
                                               (np.int16, 5, np.int8, 2, 7, False)):
        def draw(dt, g):
            lim = 128 * 2 ** g if dt == np.int16 else 128
            v = rng.integers(-lim, lim, size=4096).astype(dt)
            v[:4] = [-lim, lim - 1, 0, -1]                                  # both ends of the range meet each other below
            return v
        x, y = draw(x_dtype, gx), draw(y_dtype, gy)
        g = max(0, gx, gy)
        wide_ref, narrow_ref = add_resident_ref(x, gx, y, gy, g, ib, relu)
        wide, narrow = lr.add_resident(_t(x), gx, _t(y), gy, g, ib, relu)
        assert wide.dtype == torch.int16 and narrow.dtype == torch.int8
        assert np.array_equal(wide.numpy(), wide_ref) and np.array_equal(narrow.numpy(), narrow_ref), (gx, gy, ib, relu)


def test_histogram_and_absmax_equal_the_oracle_on_bin_edges(oracle):
    """Values on bin edges, one ulp to either side, zeros (not counted), quotients at and beyond the last bin, inf and nan; a
    power-of-two interval (what the GPU rows use), the calibration's max / 2048 + 1e-12, and one that divides inexactly."""
    for iv in (np.float32(0.125), oracle.interval(np.float32(37.5)), np.float32(0.3)):
        iv = np.float32(iv)
        edges = np.arange(0, 2052, dtype=np.float32) * iv
        x = np.concatenate([edges, np.nextafter(edges, np.float32(np.inf)), np.nextafter(edges, np.float32(-np.inf)), -edges,
                            [0.0, -0.0, 1e30, -1e30, np.inf, -np.inf, np.nan]]).astype(np.float32)
        ref = oracle.hist2048(x, iv)
        got = lr.hist2048(_t(x), float(iv))
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), ref), iv
        # accumulated onto existing counts, interval as a tensor
        again = lr.hist2048(_t(x[::3]), torch.tensor(iv), hist=got)
        assert np.array_equal(again.numpy(), oracle.hist2048(x[::3], iv, hist=ref.copy()))
    x = np.array([3.0, -7.5, 0.0, 7.25], np.float32)
    assert float(lr.absmax(_t(x))) == float(oracle.absmax(x)) == 7.5
    assert float(lr.absmax(_t(x), torch.tensor(9.0))) == float(oracle.absmax(x, 9.0)) == 9.0
    assert float(lr.absmax(_t(-x[:1]))) == 3.0


def test_layout_and_pooling_helpers_equal_numpy(oracle):
    rng = np.random.default_rng(11)
    q = rng.integers(-128, 128, size=(3, 5, 7, 32)).astype(np.int8)
    q16 = rng.integers(-32768, 32768, size=(3, 5, 7, 32)).astype(np.int16)
    for arr, g in ((q, 3), (q16, 8), (q, -2)):
        ref = oracle.dequantity(arr[..., :19].astype(np.float32), g).transpose(0, 3, 1, 2)
        assert np.array_equal(lr.dequant_nhwc_to_nchw(_t(arr), g, 19).numpy(), ref)
        s = arr[..., :19].astype(np.int64).sum(axis=(1, 2)).astype(np.float32)
        ref = (s * np.float32(2.0 ** -g)) / np.float32(35)
        assert np.array_equal(lr.avgpool_global_nhwc(_t(arr), g, 19).numpy(), ref)
    x = (rng.integers(-1200, 1200, size=(2, 19, 5, 7)) * 0.25).astype(np.float32)
    got = lr.quantize_i8_nhwc(_t(x), 1, 32).numpy()
    assert np.array_equal(got[..., :19], oracle.quantity(x, 1).astype(np.int8).transpose(0, 2, 3, 1)) and not got[..., 19:].any()
    # max pooling of the integers: padding never wins, windows clipped to the plane
    pooled = lr.maxpool_nhwc(_t(q), 3, 2, 1).numpy()
    pad = np.pad(q.astype(np.int32), ((0, 0), (1, 1), (1, 1), (0, 0)), constant_values=-1000)
    ref = np.stack([[pad[:, 2 * p:2 * p + 3, 2 * c:2 * c + 3].max(axis=(1, 2)) for c in range(4)] for p in range(3)])
    assert np.array_equal(pooled, ref.transpose(2, 0, 1, 3).astype(np.int8))


def test_matmul_convolutions_equal_the_integer_oracle(oracle):
    """The tap-by-tap fp32 matmul form on integer-valued data whose partial sums stay below 2^24: the oracle's exact integer
    convolution plus the bias."""
    rng = np.random.default_rng(3)
    x = rng.integers(-8, 9, size=(3, 20, 9, 7)).astype(np.int32)
    b = rng.integers(-50, 51, size=12).astype(np.float32)
    for (r, stride, pad) in ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0)):
        w = rng.integers(-8, 9, size=(12, 20, r, r)).astype(np.int32)
        assert np.abs(w).sum(axis=(1, 2, 3)).max() * 8 + 50 < 2 ** 24
        ref = oracle.conv2d_int(x, w, (stride, stride), (pad, pad), (1, 1)).astype(np.float32) + b.reshape(1, -1, 1, 1)
        xt, wt = _t(x.astype(np.float32)), _t(w.astype(np.float32))
        got = lr.conv1x1_f32(xt, wt[:, :, 0, 0], _t(b), stride) if r == 1 else lr.conv_kxk_f32(xt, wt, _t(b), stride, pad)
        assert np.array_equal(got.numpy(), ref), (r, stride, pad)


def test_depthwise_taps_equal_the_integer_oracle(oracle):
    rng = np.random.default_rng(5)
    x = rng.integers(-128, 128, size=(2, 19, 9, 7)).astype(np.int32)
    for r, stride, pad in ((3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 0), (3, 1, 2)):
        w = rng.integers(-128, 128, size=(19, 1, r, r)).astype(np.int32)
        ref = oracle.conv2d_int(x, w, (stride, stride), (pad, pad), (1, 1), groups=19).astype(np.float32)
        got = lr.dwconv_taps(_t(x.astype(np.float32)), _t(w.astype(np.float32)), stride, pad)
        assert np.array_equal(got.numpy(), ref), (r, stride, pad)


def test_grouped_taps_equal_the_integer_oracle(oracle):
    rng = np.random.default_rng(6)
    x = rng.integers(-128, 128, size=(2, 20, 9, 7)).astype(np.int32)
    for r, stride, pad in ((3, 1, 1), (3, 2, 1), (1, 1, 0), (1, 2, 0), (3, 1, 2)):
        w = rng.integers(-128, 128, size=(60, 4, r, r)).astype(np.int32)
        ref = oracle.conv2d_int(x, w, (stride, stride), (pad, pad), (1, 1), groups=5).astype(np.float32)
        got = lr.gconv_taps(_t(x.astype(np.float32)), _t(w.astype(np.float32)), 5, stride, pad)
        assert np.array_equal(got.numpy(), ref), (r, stride, pad)


def test_first_mismatch_names_the_index_and_the_2_31_byte_multiple():
    a = torch.zeros(4, 8)
    b = a.clone()
    assert lr.first_mismatch(a, b, 0, 4) is None
    b[2, 3] = 1
    msg = lr.first_mismatch(a, b, 2 ** 29 + 5, 4)
    assert "flat index %d" % (2 ** 29 + 5 + 19) in msg and "behind 1 x 2^31 bytes" in msg and "1 of 32" in msg
    n = torch.full((3,), float("nan"))
    assert lr.first_mismatch(n, n.clone(), 0, 4) is None
