"""The resident NewAdd of include/fq.h (fq_add_resident and every kernel that fuses it) as exact integer arithmetic: the
reference side of tests/test_gpu_add_forms.py, anchored to the CPU oracle's fp32 chain by tests/test_add_rule_cpu.py.  No float
appears below, and nothing of the library does.

    add_rule(x, y, gx, gy, ib, relu, g_wide)      -> (wide int16 or None, narrow int8), NumPy arrays or torch tensors alike
    boundary_pairs(x_bytes, y_bytes, gx, gy, ib)  -> (x, y) int64 NumPy arrays: the operand pairs at which the forms can go wrong;
                                                     scripts/add_forms_check.cpp builds the same set in C++

The rule.  x and y are int8 / int16 integers standing for x * 2^-gx and y * 2^-gy, gx, gy, ib in [-16, 16].  On the common grid
2^-16 they are X = x * 2^(16 - gx) and Y = y * 2^(16 - gy), integers below 2^47.  Then
    S      = clip(X + Y, relu ? 0 : -128 * 2^16, 127 * 2^16)       NewAdd's Sp clamp of the VALUE to [-128, 127] (and the ReLU)
    wide   = S / 2^(16 - g_wide)                                   exact: the remainder is asserted to be zero
    narrow = clip(rne(S / 2^(16 - ib)), -128, 127)                 rne: round half to even, on integers

Why this is the reference's fp32 expression clamp(x * 2^-gx + y * 2^-gy) -> max(., 0) -> clamp(rint(. * 2^ib)) bit for bit:
  * x * 2^-gx and y * 2^-gy are exact in fp32 (at most 16 significant bits times a power of two, no overflow or underflow);
  * a sum inside the clamp range is a multiple of 2^-16 of magnitude at most 128, an integer of at most 7 + 16 + 1 = 24 bits on
    that grid: representable, so the fp32 addition returns it exactly;
  * a sum outside the range may round, but rounding is monotone and both bounds are representable: it cannot come back inside,
    and the clamp returns the bound either way;
  * the scale by 2^ib is exact (s is a multiple of 2^-16 below 2^7, ib >= -16), and rint rounds half to even."""
import numpy as np

GRID = 16
LO, HI = -128 << GRID, 127 << GRID


def _is_torch(a):
    return not isinstance(a, np.ndarray)


def _i64(a):
    if _is_torch(a):
        import torch
        return a.to(torch.int64)
    return a.astype(np.int64)


def _cast(a, bits):
    if _is_torch(a):
        import torch
        return a.to(torch.int8 if bits == 8 else torch.int16)
    return a.astype(np.int8 if bits == 8 else np.int16)


def clamped_sum(x, y, gx, gy, relu):
    """S on the grid 2^-16, int64."""
    assert -16 <= gx <= 16 and -16 <= gy <= 16
    return ((_i64(x) << (GRID - gx)) + (_i64(y) << (GRID - gy))).clip(0 if relu else LO, HI)


def rne_shift(S, sh):
    """round-half-to-even of S / 2^sh for sh >= 0, on integers: the floor, the dropped bits against one half, a tie by parity."""
    if sh == 0:
        return S
    fl, rem, half = S >> sh, S & ((1 << sh) - 1), 1 << (sh - 1)
    return fl + ((rem > half) | ((rem == half) & ((fl & 1) == 1)))


def add_rule(x, y, gx, gy, ib, relu, g_wide=None):
    """(wide, narrow) of the resident NewAdd.  g_wide None: no wide output (the ABI has none where max(0, gx, gy) > 8)."""
    assert -16 <= ib <= 16
    S = clamped_sum(x, y, gx, gy, relu)
    wide = None
    if g_wide is not None:
        assert g_wide == max(0, gx, gy) and g_wide <= 8, "the ABI's wide grid"
        sh = GRID - g_wide
        assert not bool((S & ((1 << sh) - 1)).any()), "the sum is not on the grid 2^-g_wide"
        wide = _cast(S >> sh, 16)
    narrow = _cast(rne_shift(S, GRID - ib).clip(-128, 127), 8)
    return wide, narrow


# ---------------------------------------------------------------- the boundary operand set
BASE8 = (-128, -127, -1, 0, 1, 126, 127)
BASE16 = BASE8 + (-32768, -32767, -129, 128, 32766, 32767)
TIES = (-129, -128, -2, -1, 0, 1, 126, 127)          # narrow values t whose upper tie t + 1/2 is aimed at
DELTAS = (-1, 0, 1)


def base_values(nbytes):
    return BASE8 if nbytes == 1 else BASE16


def targets(ib):
    """Sums on the grid 2^-16 to aim at: the three clamp bounds, then the exact ties (t + 1/2) * 2^-ib of the narrow rounding
    (none at ib = 16, where nothing is dropped)."""
    t = [LO, 0, HI]
    if ib < GRID:
        t += [(2 * v + 1) << (GRID - 1 - ib) for v in TIES]
    return t


def boundary_pairs(x_bytes, y_bytes, gx, gy, ib):
    """Both ends of each type and their neighbours, 0 and +-1 (every pair of them); for every such value of one operand the value
    of the other that puts X + Y on a target, and the ones beside it -- where one exists in the operand's type."""
    bx = np.array(base_values(x_bytes), dtype=np.int64)
    by = np.array(base_values(y_bytes), dtype=np.int64)
    T = np.array(targets(ib), dtype=np.int64)
    D = np.array(DELTAS, dtype=np.int64)
    xs, ys = [np.repeat(bx, len(by))], [np.tile(by, len(bx))]

    def solve(fixed, g_fixed, g_free, free_bytes):
        need = T[:, None] - (fixed[None, :] << (GRID - g_fixed))               # [target][fixed value]
        sh = GRID - g_free
        v = (need >> sh)[:, :, None] + D[None, None, :]
        lim = 128 if free_bytes == 1 else 32768
        ok = ((need & ((1 << sh) - 1)) == 0)[:, :, None] & (v >= -lim) & (v < lim)
        return np.broadcast_to(fixed[None, :, None], v.shape)[ok], v[ok]

    fx, vy = solve(bx, gx, gy, y_bytes)
    xs.append(fx); ys.append(vy)
    fy, vx = solve(by, gy, gx, x_bytes)
    xs.append(vx); ys.append(fy)
    return np.concatenate(xs), np.concatenate(ys)
