"""tests/int_conv_ref.py against the project's oracle (no GPU): the float64 convolution that the large GPU cases use as their
expected value must equal oracle.conv2d_int bit for bit, and the NumPy residual add must equal the oracle's fp32 chain
DeQuantity -> NewAdd -> ReLU -> Quantity."""
import numpy as np
import pytest

from int_conv_ref import add_resident_ref, conv2d_int_fast, first_difference

# N, C, H, W, K, R, S, (stride h, w), (pad h, w), (dil h, w), fill  (fill: None = random int8, else that constant everywhere)
SHAPES = [
    (2, 16, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), None),
    (1, 64, 14, 14, 64, 1, 1, (1, 1), (0, 0), (1, 1), None),
    (3, 32, 9, 7, 40, 3, 3, (2, 2), (1, 1), (1, 1), None),
    (2, 3, 33, 31, 20, 7, 7, (2, 2), (3, 3), (1, 1), None),
    (2, 128, 7, 7, 72, 3, 3, (1, 1), (1, 1), (1, 1), None),
    (1, 256, 6, 6, 130, 1, 1, (2, 2), (0, 0), (1, 1), None),
    (2, 48, 10, 10, 33, 3, 3, (1, 1), (2, 2), (2, 2), None),          # dilation 2
    (5, 80, 5, 6, 37, 2, 3, (1, 1), (0, 0), (1, 1), None),            # R != S
    (4, 7, 11, 13, 5, 3, 2, (1, 2), (1, 0), (1, 1), None),            # R != S, strides differ, C and K prime
    (3, 13, 9, 9, 17, 1, 3, (3, 1), (0, 1), (1, 1), None),            # stride 3 down the rows only
    (2, 5, 12, 10, 11, 3, 3, (3, 3), (1, 1), (1, 1), None),           # stride 3
    (2, 19, 8, 9, 23, 3, 3, (2, 3), (2, 2), (1, 1), None),            # pad > R / 2
    (1, 9, 6, 6, 7, 3, 3, (1, 1), (3, 3), (1, 1), None),              # pad 3 with a 3 x 3 kernel: whole border rows of zeros
    (2, 11, 7, 5, 3, 1, 1, (1, 1), (2, 1), (1, 1), None),             # a padded 1 x 1 kernel
    (1, 21, 9, 8, 13, 2, 2, (2, 2), (1, 1), (2, 2), None),            # even kernel, dilation 2
    (2, 6, 10, 11, 9, 3, 5, (1, 2), (2, 3), (2, 1), None),            # R != S, dilations differ, pad > S / 2
    (3, 29, 1, 1, 31, 1, 1, (1, 1), (0, 0), (1, 1), None),            # one-pixel plane
    (2, 17, 1, 1, 6, 3, 3, (1, 1), (1, 1), (1, 1), None),             # one-pixel plane under a padded 3 x 3
    (2, 10, 1, 1, 4, 3, 3, (3, 3), (2, 2), (1, 1), None),             # ... whose outputs sample the zero border only
    (1, 1, 5, 5, 1, 3, 3, (1, 1), (1, 1), (1, 1), None),              # one channel in, one out
    (7, 2, 3, 4, 2, 3, 3, (2, 2), (1, 1), (1, 1), None),
    (1, 37, 4, 19, 41, 1, 5, (1, 2), (0, 2), (1, 2), None),
    (2, 64, 6, 6, 64, 3, 3, (1, 1), (1, 1), (1, 1), -128),            # all (-128): the largest accumulator, 576 * 2^14
    (1, 128, 5, 5, 8, 3, 3, (1, 1), (0, 0), (1, 1), -128),            # 1152 * 2^14 = 18 874 368 > 2^24 in every output
    (1, 1024, 2, 3, 5, 1, 1, (1, 1), (0, 0), (1, 1), -128),
    (2, 40, 1, 1, 9, 1, 1, (1, 1), (0, 0), (1, 1), -128),
    (1, 24, 7, 7, 10, 3, 3, (2, 2), (1, 1), (1, 1), 127),
    (2, 33, 6, 9, 12, 3, 3, (1, 1), (1, 1), (1, 1), "mixed"),         # x = -128 everywhere, w = 127 everywhere
    (1, 300, 3, 3, 3, 3, 3, (1, 1), (1, 1), (1, 1), None),            # 2700 taps
    (4, 15, 13, 3, 21, 5, 1, (2, 1), (2, 0), (1, 1), None),
]


def _operands(case):
    N, C, H, W, K, R, S, _st, _pd, _dl, fill = case
    rng = np.random.default_rng(sum(case[:7]) * 31 + R)
    if fill is None:
        x = rng.integers(-128, 128, size=(N, C, H, W)).astype(np.int32)
        w = rng.integers(-128, 128, size=(K, C, R, S)).astype(np.int32)
        x.flat[::11] = -128
        w.flat[::7] = -128
    elif fill == "mixed":
        x = np.full((N, C, H, W), -128, dtype=np.int32)
        w = np.full((K, C, R, S), 127, dtype=np.int32)
    else:
        x = np.full((N, C, H, W), fill, dtype=np.int32)
        w = np.full((K, C, R, S), fill, dtype=np.int32)
    return x, w


def test_the_shape_list_covers_what_it_claims():
    cs = SHAPES
    assert len(cs) >= 30
    assert {s for c in cs for s in c[7]} == {1, 2, 3} and {p for c in cs for p in c[8]} == {0, 1, 2, 3}
    assert {d for c in cs for d in c[9]} == {1, 2}
    assert any(c[5] != c[6] for c in cs) and any(c[7][0] != c[7][1] for c in cs) and any(c[9][0] != c[9][1] for c in cs)
    assert any(2 * c[8][0] > c[5] for c in cs) and any(2 * c[8][1] > c[6] for c in cs)               # pad > R / 2
    assert sum(1 for c in cs if c[1] % 8 and c[4] % 8) >= 8                                          # ragged C and K
    assert sum(1 for c in cs if (c[2], c[3]) == (1, 1)) >= 3
    assert sum(1 for c in cs if c[10] == -128) >= 3
    assert any(c[10] == -128 and c[5] * c[6] * c[1] * 2 ** 14 > 2 ** 24 for c in cs)                 # beyond fp32's integers


@pytest.mark.parametrize("case", SHAPES, ids=["%dx%dx%dx%d-k%d-%dx%d-s%s-p%s-d%s-%s" % c for c in SHAPES])
def test_the_float64_convolution_equals_the_oracle_bit_for_bit(oracle, case):
    _N, C, _H, _W, _K, R, S, st, pd, dl, fill = case
    x, w = _operands(case)
    ref = oracle.conv2d_int(x, w, st, pd, dl)
    got = conv2d_int_fast(x, w, st, pd, dl)
    assert got.dtype == np.int64 and got.shape == ref.shape
    assert np.array_equal(got, ref), first_difference(got, ref)
    if fill == -128 and not any(pd):
        assert int(got.max()) == R * S * C * 2 ** 14 == int(got.min())                               # the bound itself


def test_the_float64_convolution_refuses_what_it_cannot_hold():
    x = np.zeros((1, 4, 3, 3), dtype=np.int32)
    w = np.zeros((2, 4, 1, 1), dtype=np.int32)
    x[0, 0, 0, 0] = 128
    with pytest.raises(AssertionError):
        conv2d_int_fast(x, w)                                         # not an int8 value
    with pytest.raises(AssertionError):
        conv2d_int_fast(np.zeros((1, 4, 3, 3), dtype=np.float32), w)
    with pytest.raises(AssertionError):
        conv2d_int_fast(np.zeros((1, 3, 3, 3), dtype=np.int32), w)    # channel counts differ


@pytest.mark.parametrize("xb,gx,yb,gy,ib,relu", [(1, 3, 1, 5, 4, True), (1, 5, 2, 5, 3, True), (2, 6, 1, 2, 6, False),
                                                 (2, 8, 2, 7, 5, True), (1, -1, 1, 2, 0, False), (1, 0, 2, 0, 1, True),
                                                 (1, 3, 2, 6, 4, False), (1, 4, 1, 4, -1, True)])
def test_the_numpy_residual_add_equals_the_oracles_fp32_chain(oracle, xb, gx, yb, gy, ib, relu):
    rng = np.random.default_rng(xb * 1000 + gx * 100 + yb * 10 + gy)
    shape = (3, 5, 7, 32)

    def operand(bytes_, g):
        v = rng.integers(-128, 128, size=shape)
        if bytes_ == 2:
            v = (v * rng.integers(1, 2 ** max(g, 0) + 1, size=shape)).clip(-128 * 2 ** max(g, 0), 127 * 2 ** max(g, 0))
        v.flat[:4] = [v.min(), v.max(), 0, -1]
        return v.astype(np.int8 if bytes_ == 1 else np.int16)

    x, y = operand(xb, gx), operand(yb, gy)
    g = max(0, gx, gy)
    s = oracle.add_sat(oracle.dequantity(x.astype(np.float32), gx), oracle.dequantity(y.astype(np.float32), gy))
    if relu:
        s = np.maximum(s, np.float32(0))
    exact = s.astype(np.float64) * 2.0 ** g
    assert np.all(exact == np.rint(exact))
    wide, narrow = add_resident_ref(x, gx, y, gy, g, ib, relu)
    assert wide.dtype == np.int16 and narrow.dtype == np.int8
    np.testing.assert_array_equal(wide, exact.astype(np.int16))
    np.testing.assert_array_equal(narrow, oracle.quantity(s, ib).astype(np.int8))


def test_first_difference_names_the_output_and_its_tile():
    ref = np.zeros((3, 5, 10, 20), dtype=np.int32)
    assert first_difference(ref, ref.copy()) is None
    got = ref.copy()
    got[1, 3, 4, 7] = 9                                               # m = (1 * 10 + 4) * 20 + 7 = 287 -> tile 2
    got[2, 0, 9, 19] = 1
    msg = first_difference(got, ref)
    assert msg.startswith("2 of 3000 outputs differ; first at (n, k, p, q) = (1, 3, 4, 7), pixel tile m // 128 = 2: got 9, expected 0"), msg
    assert "2 pixel tiles affected (first 2, last 4), channels 0..3" in msg, msg
    assert "shape" in first_difference(ref[:1], ref)
