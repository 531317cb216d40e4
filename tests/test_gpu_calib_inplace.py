"""The fused calibration forward under in-place writes: identical tables or a raise, never a silently different histogram.

Which kernel is handed which tensor is decided by host bookkeeping over tensor identity and version counters (the poison probe,
ctl.pair_ok, ctl.pairs / ctl.sum_relu, the cache entry; tools/_fused_forward.py, tools/_hook_state.py, tools/pytorch_quantizer.py).
calib_inplace_nets.chain_net is a chain of three residual sums whose forward writes to one of its own tensors in place at a
chosen site -- in every forward ("always": the probe forwards can know), or only from the second batch on ("later": they cannot).

The reference is the product's plainest path on the same convolution kernels (calib_inplace_nets.ARMS["reference"]): every
tensor counted from inside its hook, i.e. the value its module returned, which is what the reference's hook copies to the host
(pytorch_quantizer.py:509-513, _EagerStats' docstring) -- pinned here against clones taken at hook time and the CPU oracle.
Maxima are maxima and histograms integer counts: every comparison is for equality, no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

from tools._hook_state import _AFTER_FORWARD
from calib_inplace_nets import ARMS, BATCH_SHAPE, N_BATCHES, SITES, calibrate_chain

pytestmark = pytest.mark.gpu

_SHORTCUT = "written to after the add that pass 1 left to pass 2"        # _add_with_pairs, where pass 2 reads a pair's shortcut
_KEPT = "modified in place after its statistics were taken"             # _kept_intact, where pass 1 puts a forward into the cache
_PENDING = "modified in place before its statistics were taken"         # _EagerStats.flush, the grouped launch after a forward

# (site, when) -> what each arm under test must do, in the order of _ARMS.  "equal": the reference arm's table, bits, maxima and
# histograms; anything else: RuntimeError with that message.  Reasons, by the code:
#   always   the trace and the probe forwards meet the same writes as every batch.  A write to a ReLU output is invisible to the
#            version counters of the HOOKED tensors, and must be absorbed by the pair bookkeeping; a write to a hooked tensor makes the
#            probe report an in-place consumer, and the calibration runs without cache, deferral or grouped launches.
#   later    relu_before_add*: the shortcut is no longer max(the sum in front, 0) -- it stays a kept tensor, with the version it had
#            at the add.  relu_after_next_add: a chain link re-makes the shortcut from the pair in front, which IS what the add saw
#            (equal); kept as a tensor (pair_chain off) it no longer is, and its version says so where pass 2 reads it.
#            A hooked tensor written after its producer took the maximum would reach pass 2 overwritten: refused when the forward
#            is put into the cache -- except the shortcut of a pair, which has its own check where pass 2 reads it, and except a sum
#            left to its pair: pass 1 never wrote that tensor, the cache does not hold it, the write lands in memory nobody reads.
_ARMS = ("A", "B", "A_flat")
EXPECT = {
    ("none", "always"): ("equal", "equal", "equal"),
    ("relu_before_add", "always"): ("equal", "equal", "equal"),
    ("relu_before_add", "later"): ("equal", "equal", "equal"),
    ("relu_before_add_module", "always"): ("equal", "equal", "equal"),
    ("relu_before_add_module", "later"): ("equal", "equal", "equal"),
    ("relu_view_before_add", "always"): ("equal", "equal", "equal"),
    ("relu_view_before_add", "later"): ("equal", "equal", "equal"),
    ("relu_after_next_add", "always"): ("equal", "equal", "equal"),
    ("relu_after_next_add", "later"): ("equal", "equal", _SHORTCUT),
    ("conv3_after_add", "always"): ("equal", "equal", "equal"),
    ("conv3_after_add", "later"): (_KEPT, _KEPT, _KEPT),
    ("sum_after_relu", "always"): ("equal", "equal", "equal"),
    ("sum_after_relu", "later"): ("equal", "equal", "equal"),
    ("c1_after_relu", "always"): ("equal", "equal", "equal"),
    ("c1_after_relu", "later"): (_KEPT, _KEPT, _KEPT),
    ("projection_after_add", "always"): ("equal", "equal", "equal"),
    ("projection_after_add", "later"): (_SHORTCUT, _SHORTCUT, _SHORTCUT),
}
_CASES = [(site, when, arm) for (site, when) in EXPECT for arm in _ARMS]
_SHORTCUT_BYTES = BATCH_SHAPE[0] * 128 * (BATCH_SHAPE[2] // 2) * (BATCH_SHAPE[3] // 2) * 4      # one block input behind b1


def test_the_table_of_outcomes_is_complete_and_only_a_late_write_may_be_refused():
    assert set(s for s, _w in EXPECT) == set(SITES) and set(_ARMS) | {"reference"} == set(ARMS)
    assert set(EXPECT) == set((s, w) for s in SITES for w in ("always", "later") if (s, w) != ("none", "later"))
    for (site, when), outcomes in EXPECT.items():
        assert len(outcomes) == len(_ARMS) and all(o in ("equal", _SHORTCUT, _KEPT) for o in outcomes)
        if when == "always" or site in ("none", "relu_before_add", "relu_before_add_module", "relu_view_before_add", "sum_after_relu"):
            assert outcomes == ("equal",) * 3, (site, when)
    assert EXPECT[("projection_after_add", "later")][0] == _SHORTCUT


@functools.lru_cache(maxsize=None)
def _reference(site, when):
    """Computed once per (site, when), shared by its arms, never changed."""
    return calibrate_chain(site, when, "reference")


@functools.lru_cache(maxsize=None)
def _clean(arm):
    """The clean twin under the same arm (what the counters and the cache's size are compared with)."""
    return calibrate_chain("none", "always", arm)


def _assert_equal(got, want):
    assert got["table"] == want["table"] and got["bits"] == want["bits"]
    assert got["max"] == want["max"]                                    # every abs-max, bit for bit
    rows = [n for n, r in sorted(want["row"].items(), key=lambda e: e[1])
            if not torch.equal(got["hist"][got["row"][n]], want["hist"][r])]
    assert not rows, "histograms differ from the reference arm's: %s" % rows


@pytest.mark.parametrize("site,when,arm", _CASES, ids=["%s-%s-%s" % c for c in _CASES])
def test_identical_tables_or_a_raise(site, when, arm):
    expect = EXPECT[(site, when)][_ARMS.index(arm)]
    if expect != "equal":
        assert when == "later"
        with pytest.raises(RuntimeError, match=expect):
            calibrate_chain(site, when, arm)
        return
    got = _clean(arm) if site == "none" else calibrate_chain(site, when, arm)
    t = got["timings"]
    print(site, when, arm, dict((k, t.get(k)) for k in ("conv_add_chains_proven", "conv_add_launches", "sums_left_to_pass2_pairs",
                                                     "pairs_chained", "cache_bytes", "cached_batches", "inplace_consumers")))
    _assert_equal(got, _reference(site, when))
    assert t["inplace_consumers"] or (t["cache_plan"]["kind"] == ARMS[arm][1] and t["cache_bytes"] > 0)
    if site == "none":
        # the fusions were really taken: three proven tails, their sums left to pass 2, b2 and b3 as chain links
        assert t["conv_add_chains_proven"] == 3 and t["inplace_consumers"] is False
        assert t["sums_left_to_pass2_pairs"] > 0 and t["sums_left_to_pass2_pairs"] == t["conv_add_launches"]
        if arm == "A_flat":
            assert t["pairs_chained"] == 0
        else:
            assert t["pairs_chained"] * 3 == t["sums_left_to_pass2_pairs"] * 2
            flat = _clean("A_flat")["timings"]
            assert flat["sums_left_to_pass2_pairs"] == t["sums_left_to_pass2_pairs"]
            # ... and a chain link's shortcut is not in the cache: two block inputs per batch with pairs less than the flat form
            assert flat["cache_bytes"] - t["cache_bytes"] >= t["pairs_chained"] * _SHORTCUT_BYTES
    if site.startswith("relu_before_add") or (site, when) == ("relu_after_next_add", "later"):
        clean = _clean(arm)["timings"]
        assert t["conv_add_chains_proven"] == 3 and t["inplace_consumers"] is False
        assert t["sums_left_to_pass2_pairs"] == clean["sums_left_to_pass2_pairs"] > 0           # the pair path ran ...
    if site.startswith("relu_before_add"):
        if arm == "A_flat":
            assert t["pairs_chained"] == 0 and t["cache_bytes"] == clean["cache_bytes"]       # (every shortcut is kept anyway)
        else:
            # ... and b2's pair fell back to a kept shortcut, which b3 is still chained behind
            assert 0 < t["pairs_chained"] < clean["pairs_chained"]
            assert t["cache_bytes"] - clean["cache_bytes"] == (clean["pairs_chained"] - t["pairs_chained"]) * _SHORTCUT_BYTES
    if (site, when) in (("relu_after_next_add", "later"), ("sum_after_relu", "later")):
        clean = _clean(arm)["timings"]                                   # the write changes nothing the cache holds: the clean twin's
        assert all(t[k] == clean[k] for k in ("sums_left_to_pass2_pairs", "pairs_chained", "cache_bytes", "conv_add_chains_proven"))


@pytest.mark.parametrize("site", SITES)
def test_the_reference_arm_counts_what_each_module_returned(site, oracle):
    """The reference arm itself, once per site under "always": forward hooks of this test's own clone every cared module's output
    when the module returns it (after the calibration's hook of the same call, whose kernel fills the tensor).  Every abs-max of
    the arm is the clones' maximum, and the histogram rows of b2's and b3's sums and of b2's last convolution are the CPU oracle's
    histogram of the clones with the collector's interval."""
    tape = {}
    got = calibrate_chain(site, "always", "reference", tape=tape)
    want = _reference(site, "always")
    _assert_equal(got, want)                                            # (this test's hooks change nothing)
    keys = sorted(set(k for _i, k in tape))
    assert set(keys) == set(got["row"]) - {"image"} and len(tape) == N_BATCHES * len(keys)
    for key in keys:
        top = max(float(tape[(i, key)].abs().max()) for i in range(N_BATCHES))
        assert float(got["max"][key]) == top, key
    for module in ("b2.add", "b3.add", "b2.c3"):
        key = got["key"][module]
        hist = np.zeros(2048, dtype=np.int64)
        for i in range(N_BATCHES):
            oracle.hist2048(tape[(i, key)].cpu().numpy(), got["interval"][key], hist=hist)
        assert int(hist.sum()) == N_BATCHES * tape[(0, key)].numel()
        assert np.array_equal(got["hist"][got["row"][key]].numpy(), hist), (module, key)


def test_a_late_write_to_a_tensor_whose_statistics_wait_for_the_grouped_launch_is_refused():
    """stats_group_bytes at its default: when no producer takes a tensor's statistic (fuse_bias_absmax off), the hooked tensors
    wait for ONE launch after the forward -- which the probe forward allowed, having seen no in-place write.  A model that starts
    to write later is refused by that launch's own look at the version counters."""
    with pytest.raises(RuntimeError, match=_PENDING):
        calibrate_chain("c1_after_relu", "later", "A", fuse_bias_absmax=False)
    # (the clean twin under the same switches calibrates, in that very mode: one launch per forward, every batch cached)
    t = calibrate_chain("none", "always", "A", fuse_bias_absmax=False)["timings"]
    assert t["stats_group_bytes"] == _AFTER_FORWARD and t["cached_batches"] == N_BATCHES and t["inplace_consumers"] is False
