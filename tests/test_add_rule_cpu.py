"""The resident NewAdd without a GPU: the integer rule of tests/add_rule.py held against the CPU oracle's fp32 chain over every
(gx, gy, ib) of the ABI, the host check of the form selection and of each form's range argument (scripts/add_forms_check.cpp,
built with the address and undefined-behaviour sanitizers), and the conditions the GPU tests' case list meets by construction.
Every comparison is exact.  No GPU kernel and nothing of csrc/fq_resident.h takes part in the first of these."""
import os
import subprocess

import numpy as np
import pytest

import add_form_cases as ac
import add_rule as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE = range(-16, 17)


@pytest.mark.parametrize("gx", RANGE)
def test_the_rule_is_the_oracle_chain_on_every_grid(oracle, gx):
    """DeQuantity -> NewAdd (Sp clamp) -> ReLU -> Quantity through the oracle's fp32 functions, on the boundary operand set of an
    int16 x and an int16 y (which holds the int8 one): the rule's narrow output is that chain's, and for g <= 8 its wide output is
    the exact s * 2^g."""
    checked = 0
    for gy in RANGE:
        g = max(0, gx, gy)
        for ib in RANGE:
            x, y = ar.boundary_pairs(2, 2, gx, gy, ib)
            s = oracle.add_sat(oracle.dequantity(x.astype(np.float32), gx), oracle.dequantity(y.astype(np.float32), gy))
            for relu in (False, True):
                sr = np.maximum(s, np.float32(0)) if relu else s
                wide, narrow = ar.add_rule(x, y, gx, gy, ib, relu, g if g <= 8 else None)
                assert narrow.dtype == np.int8 and np.array_equal(narrow.astype(np.float32), oracle.quantity(sr, ib)), (gx, gy, ib, relu)
                if g <= 8:
                    assert wide.dtype == np.int16 and np.array_equal(wide.astype(np.float64), sr.astype(np.float64) * 2.0 ** g)
                else:
                    assert wide is None
                checked += x.size
    assert checked > 33 * 33 * 2 * 169


def test_the_boundary_set_holds_what_it_claims():
    """Both ends of each type and their neighbours, 0 and +-1 on every set; on sets whose operands can reach them, sums on each
    clamp bound and one step beside it, and exact ties of the narrow rounding with an even and with an odd floor."""
    lim = {1: 128, 2: 32768}
    for (xb, yb, gx, gy, ib) in ((1, 2, 4, 5, 4), (1, 1, 0, 0, -3), (2, 2, 0, 8, -3), (2, 1, 3, -2, 1), (2, 1, -16, 16, 16), (1, 2, 16, -16, -16)):
        x, y = ar.boundary_pairs(xb, yb, gx, gy, ib)
        assert x.min() == -lim[xb] and x.max() == lim[xb] - 1 and y.min() == -lim[yb] and y.max() == lim[yb] - 1
        for v in (-lim[xb], 1 - lim[xb], -1, 0, 1, lim[xb] - 2, lim[xb] - 1):
            assert (x == v).any()
        for v in (-lim[yb], 1 - lim[yb], -1, 0, 1, lim[yb] - 2, lim[yb] - 1):
            assert (y == v).any()
        if abs(gx) == 16:
            continue                                                        # (the ends of the ABI: nothing lands on a bound there)
        total = (x << (16 - gx)) + (y << (16 - gy))
        step = 1 << (16 - min(gx, gy))                                      # the coarser operand's grid step
        for bound in (ar.LO, 0, ar.HI):
            off = np.abs(total - bound)
            assert (off == 0).any() and ((off > 0) & (off <= step)).any(), (gx, gy, ib, bound)
        sh = 16 - ib
        tie = ((total & ((1 << sh) - 1)) == (1 << (sh - 1))) & (total > ar.LO) & (total < ar.HI)
        assert (tie & ((total >> sh) & 1 == 0)).any() and (tie & ((total >> sh) & 1 == 1)).any(), (gx, gy, ib)


def test_rne_shift_on_every_small_integer():
    """The rounding of the rule against Python's round() (half to even) on exact fractions."""
    from fractions import Fraction
    v = np.arange(-1100, 1100, dtype=np.int64)
    for sh in (0, 1, 2, 3, 7):
        assert ar.rne_shift(v, sh).tolist() == [round(Fraction(int(a), 1 << sh)) for a in v]


@pytest.fixture(scope="module")
def forms_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("add_forms") / "add_forms_check")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "scripts", "add_forms_check.cpp")])
    return exe


def test_selection_and_range_arguments_on_the_host(forms_check):
    """The program's own header says what it walks.  Every parameter set is visited, every form is selected somewhere, and the
    fp32 chain and the 32-bit form also run beside the selection wherever their preconditions hold."""
    env = {k: v for k, v in os.environ.items() if k not in ("FQ_ADD_FLOAT", "FQ_ADD_PACKED")}      # (they override the selection)
    out = subprocess.run([forms_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    assert out.returncode == 0 and out.stdout.startswith("add_forms_check: OK 287496 sets") and not out.stderr, out.stdout + out.stderr
    words = out.stdout.split()
    selected = [int(words[words.index(n) + 1].rstrip(",")) for n in ("fp32", "int32", "int32_shift", "packed")]
    assert sum(selected) == 33 ** 3 * 2 * 4 and min(selected) > 0
    beside = [int(w) for w in words[-4:]]
    assert beside[0] == sum(selected[1:]) and beside[2] == selected[3] and beside[1] == beside[3] == 0


def test_the_program_walks_the_operand_set_of_the_rule(forms_check):
    for (xb, yb, gx, gy, ib) in ((1, 2, 4, 5, 4), (1, 1, 4, 4, 4), (2, 2, 0, 8, -3), (2, 1, -16, 16, 16), (1, 2, 16, -16, -16), (2, 2, 8, 8, 0)):
        out = subprocess.run([forms_check, "pairs"] + [str(v) for v in (xb, yb, gx, gy, ib)], stdout=subprocess.PIPE, check=True,
                             universal_newlines=True).stdout
        got = np.array([[int(v) for v in line.split()] for line in out.splitlines()], dtype=np.int64)
        x, y = ar.boundary_pairs(xb, yb, gx, gy, ib)
        assert np.array_equal(got[:, 0], x) and np.array_equal(got[:, 1], y)


# ---------------------------------------------------------------- the case list of tests/test_gpu_add_forms.py
@pytest.fixture(scope="module")
def form_of():
    from common.quantity import _native
    return _native.add_resident_form


def test_add_resident_form_follows_the_selection(form_of):
    """The diagnostic against the selection's conditions as include/fq.h's callers know them, on every parameter set."""
    from common.quantity import _native
    for gx in RANGE:
        for gy in RANGE:
            for ib in RANGE:
                q = ac.quantities(gx, gy, ib)
                int_ok = q["g"] <= 8 and q["shx"] <= 12 and q["shy"] <= 12 and -15 <= q["k"] <= 24
                for (xb, yb) in ac.TYPE_PAIRS:
                    packed = int_ok and xb == 1 and 1 <= q["k"] <= 8 and q["shx"] <= 8 and (q["shy"] <= 8 if yb == 1 else q["shy"] == 0)
                    want = 3 if packed else ((2 if q["k"] > 0 else 1) if int_ok else 0)
                    assert form_of(xb, gx, yb, gy, ib, 0) == form_of(xb, gx, yb, gy, ib, 1) == want, (xb, yb, gx, gy, ib)
    for bad in ((3, 0, 1, 0, 0, 0), (1, 0, 0, 0, 0, 0), (1, 17, 1, 0, 0, 0), (1, 0, 1, -17, 0, 0), (1, 0, 1, 0, 17, 0)):
        assert _native.lib().fq_add_resident_form(*bad) == -1
        with pytest.raises(_native.FqError):
            form_of(*bad)
    assert sorted(_native.ADD_FORMS) == [0, 1, 2, 3]


def test_the_case_list_meets_its_conditions_by_construction(form_of):
    """The counts tests/test_gpu_add_forms.py relies on, where no GPU is needed: every form with every operand-type pair that can
    take it and with ReLU on and off, both sides of every edge, the project's own sets, and a list short enough to run."""
    sets = ac.triples()
    assert len(sets) == len(set(sets)) and 100 <= len(sets) <= 160
    assert all(-16 <= v <= 16 for s in sets for v in s)
    cov = ac.coverage(form_of)
    want = {(f, xb, yb, relu) for (xb, yb) in ac.TYPE_PAIRS for f in ac.reachable_forms(xb, yb) for relu in (0, 1)}
    assert cov["forms"] == want and len(want) == 28
    assert cov["edges"] == {(n, v) for n, vs in ac.EDGES.items() for v in vs} and len(cov["edges"]) == 28
    assert len(ac.edge_sets()) == 2 * 28 and set(ac.project_sets()) <= set(sets) and len(set(ac.project_sets())) >= 80
    # every edge of the selection is crossed where it changes the form: the two sides run different code for some operand-type pair
    for name, (a, b) in (("g", (8, 9)), ("shx", (8, 9)), ("shx", (12, 13)), ("shy", (8, 9)), ("shy", (12, 13)), ("k", (-16, -15)),
                         ("k", (0, 1)), ("k", (8, 9)), ("k", (24, 25)), ("shy", (0, 1))):
        fa, fb = ([tuple(form_of(xb, s[0], yb, s[1], s[2], 0) for n, v, s in ac.edge_sets() if (n, v) == (name, side))
                   for xb, yb in ac.TYPE_PAIRS] for side in (a, b))
        assert fa != fb, (name, a, b)


def test_the_fused_sets_cover_every_class(form_of):
    fs = ac.fused_sets(form_of)
    classes = {(form_of(1, gx, yb, gy, ib, relu), yb, relu) for (gx, gy, ib, yb, relu) in fs}
    assert classes == {(f, yb, relu) for f in ac.FORMS for yb in (1, 2) for relu in (0, 1)} and len(fs) == len(set(fs)) <= 32
    shy = {(ac.quantities(gx, gy, ib)["shy"], relu) for (gx, gy, ib, yb, relu) in fs if yb == 2}
    assert {(0, 0), (0, 1), (1, 0), (1, 1)} <= shy
    assert any(ac.quantities(*s[:3])["g"] > 8 for s in fs) and any(form_of(1, s[0], s[3], s[1], s[2], s[4]) == 0 and
                                                                  ac.quantities(*s[:3])["g"] <= 8 for s in fs)


def test_the_block_tail_sets_are_the_block_tail_tests():
    import test_gpu_block_tail as bt
    assert {c[7] for c in bt.CASES} | {c[6] for c in bt.PROJ_CASES} == set(ac.BLOCK_TAIL_TRIPLES)
