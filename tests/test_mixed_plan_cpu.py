"""Random graphs that mix every layer type a switch of resident.enable() takes, with all eight switches on, on a box without a GPU
(DESIGN section 27).  Each model of a fixed family (tests/mixed_nets.py) is calibrated with the oracle-backed engine and rebuilt as
the integer-simulation model; on the union of the oracle-backed doubles (tests/all_doubles.py) its logits with fp32 module
boundaries -- the reference's chain, which goldens G11, G16, G18, G20 and G21 pin to the reference -- are compared bit for bit with
the planned logits: on the example batch, on another batch, at another batch size, pickled, with every switch on and with each one
switch off; every hooked module is planned or named with a reason; and over the family the plans must contain the interactions
between features that no single-feature test has.  Every comparison is exact."""
import functools
import inspect
import json
import os
import pickle

import numpy as np
import pytest
import torch

import all_doubles
import depthwise_nets as dn
import mixed_nets as mn

FAMILY = mn.family()
SWITCHES = tuple(mn.ALL_SWITCHES)
PERTURBED = [i for i, _seed in FAMILY if i % 3 == 0]         # the perturbed-bits arm: about a third of the family
PER_CHANNEL = (2, 5, 7, 16)                                   # models with grouped and depthwise layers (asserted below)
TIMES = 3                                                     # every interaction is seen at least this often


def _leave_out(name):
    kw = dict(mn.ALL_SWITCHES)
    kw[name] = False
    if name == "concat":
        kw["flatten"] = False                                 # (flatten=True without concat=True is a ValueError)
    return kw


def _types(net, *names):
    return sum(1 for m in net.modules() if type(m).__name__ in names)


def _accounting(net, summary, plans, kw, tag):
    """Every hooked module is planned or named with a reason, and what the plan promises its readers holds on the graph."""
    if kw["activations"]:
        assert summary["resident_activations"] + len(plans.activations_left) == sum(
            1 for m in net.modules() if type(m).__name__ in mn.ACTIVATIONS), tag
        assert set(plans.activations_revoked) <= set(plans.activations_left), tag
    if kw["shuffle"]:
        assert summary["resident_shuffles"] + summary["resident_slices"] + len(plans.shuffle_left) == _types(net, "ChannelShuffle", "Slice"), tag
    if kw["relu6"]:
        # (one nn.ReLU6 module may serve several producers, as a shared nn.ReLU does: the counter counts fusions, so modules are
        #  counted by their instance-level forward)
        fused = sum(1 for m in net.modules() if isinstance(m, torch.nn.ReLU6) and "forward" in m.__dict__)
        assert fused + len(plans.relu6_left) == _types(net, "ReLU6"), tag
        assert plans.fused_relu6s == summary["fused_relu6s"] == sum(1 for p in plans.values() if p.clip) >= fused, tag
    f = mn.facts(net, plans)
    assert not f["pool_operand"], (tag, "a windowed pool's value is an operand of", f["pool_operand"])
    assert not f["fp32_reader"], (tag, "emit_f32 is off but fp32 is read", f["fp32_reader"])
    return f


def check_plans(net, x, x2, tag, leave_one_out=True):
    """The exact equalities and the accounting on one integer-simulation model (inside all_doubles.installed()).
    -> (summary, facts) of the plan with everything on."""
    from common.quantity import resident
    with torch.no_grad():
        want = [net(x).clone(), net(x2).clone(), net(x[:3]).clone()]
    result = None
    for kw in [dict(mn.ALL_SWITCHES)] + ([_leave_out(s) for s in SWITCHES] if leave_one_out else []):
        off = [s for s in SWITCHES if not kw[s]]
        what = "%s without %s" % (tag, off)
        summary = resident.enable(net, x, **kw)               # (verify=True: the example batch, at enable time)
        plans = resident.describe(net)
        with torch.no_grad():
            assert torch.equal(net(x), want[0]), what
            assert torch.equal(net(x2), want[1]), what + " (another batch)"
            assert torch.equal(net(x[:3]), want[2]), what + " (another batch size)"
            again = pickle.loads(pickle.dumps(net))
            assert torch.equal(again(x2), want[1]), what + " (pickled)"
            assert resident.describe(again).keys() == plans.keys(), what
        facts = _accounting(net, summary, plans, kw, what)
        if not off:
            result = (summary, facts)
        resident.disable(net)
        assert not resident.describe(net) and not any("forward" in m.__dict__ for m in net.modules()), what
        with torch.no_grad():
            assert torch.equal(net(x), want[0]), what + " (disabled)"
    return result


@functools.lru_cache(maxsize=None)
def checked(index):
    """Model `index` of the family through every check; what the coverage conditions need of it."""
    seed = dict(FAMILY)[index]
    out = {}
    with all_doubles.installed():
        info, (net,) = mn.calibrated(index, seed, [all_doubles.installed])
        x, x2 = mn.inputs(net, index, seed)
        out["summary"], out["facts"] = check_plans(net, x, x2, "model %d" % index)
        out["has"] = {"depthwise": 0, "grouped": 0}
        g = mn.Graph(net)
        for name in g.calls:
            k = g.kind(name)
            out["has"][k] = out["has"].get(k, 0) + 1
            if k == "concat" and any(g.kind(g.maker(t)[0]) == "concat" for t in g.made_by[g.out_of(name)[0]][1] if g.maker(t)[0]):
                out["has"]["nested"] = out["has"].get("nested", 0) + 1
            if k == "avgpool" and g.kind(g.readers[g.out_of(name)[0]][0]) == "view":
                out["has"]["avgpool"] -= 1                    # (the whole-plane pool in front of the head is no windowed pool)
        if index in PERTURBED:
            plain = mn.float_model(index, seed)
            other = dn.rebuild(plain, mn.perturbed(info, index, net))
            other.plan = net.plan
            out["perturbed_summary"], out["perturbed_facts"] = check_plans(other, x, x2, "model %d, perturbed bits" % index,
                                                                            leave_one_out=False)
    return out


# ---------------------------------------------------------------- 1. the stack of doubles
def test_the_installed_doubles_are_the_widest_of_each_name():
    import concat_doubles
    import depthwise_doubles
    import relu6_doubles
    from common.quantity import _native
    before = {k: getattr(_native, k) for k in all_doubles.NAMES}
    with all_doubles.installed() as nat:
        assert nat is _native
        assert all(getattr(nat, k) is not before[k] for k in all_doubles.NAMES), "every listed entry point is doubled"
        assert nat.recon_epilogue is depthwise_doubles.recon_epilogue                   # (takes per-channel shifts)
        assert nat.concat_i8_nhwc is concat_doubles.concat_i8_nhwc
        for name in ("conv2d_i8_resident", "conv2d_i8_stem", "dwconv2d_i8_resident", "gconv2d_i8_resident"):
            f = getattr(nat, name)
            assert f.__module__ == "relu6_doubles" and "clip" in inspect.signature(f).parameters, name   # the `clip=`-taking wrappers
        del relu6_doubles.calls[:]
        q = torch.zeros(1, 2, 2, 16, dtype=torch.int8)
        w = nat.pack_weight_dw(torch.ones(16, 1, 3, 3))
        nat.dwconv2d_i8_resident(q, w, torch.zeros(16), (1, 1), (1, 1), 4, 4, True, clip=nat.relu6_clip(4))
        assert relu6_doubles.calls == [("dwconv2d_i8_resident", nat.relu6_clip(4))]
    assert all(getattr(_native, k) is before[k] for k in all_doubles.NAMES), "leaving restores the library's own"


# ---------------------------------------------------------------- 2. the generator
def test_the_generator_is_seeded_small_and_pickles():
    a, b = mn.RandomMixedNet(3, 18), mn.RandomMixedNet(3, 18)
    assert a.plan == b.plan and all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert mn.RandomMixedNet(4, 18).plan != a.plan
    again = pickle.loads(pickle.dumps(a))
    x = torch.randn(a.batch, a.cin, a.size, a.size, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        assert torch.equal(again.eval()(x), a.eval()(x))
    kinds = set()
    for i, seed in FAMILY:
        m = mn.RandomMixedNet(i, seed)
        assert (m.cin, m.batch) == (3, 4) and m.size in (8, 16) and 2 <= len(m.steps) <= 6 and m.n == len(list(m.modules()))
        kinds |= set(m.steps)
    assert kinds == set(mn.STEPS), set(mn.STEPS) - kinds


# ---------------------------------------------------------------- 3. every model: exact logits, accounting
@pytest.mark.parametrize("index", [i for i, _seed in FAMILY])
def test_every_plan_keeps_the_logits_and_accounts_for_every_module(index, oracle):
    checked(index)


@pytest.mark.parametrize("index", PER_CHANNEL)
def test_per_channel_bits_on_the_grouped_and_depthwise_layers(index, oracle):
    seed = dict(FAMILY)[index]
    with all_doubles.installed():
        info, (net,) = mn.calibrated(index, seed, [all_doubles.installed], per_channel=True)
        assert any(isinstance(v["weight_bit"], list) for v in info.values()), "the model has no grouped or depthwise layer"
        x, x2 = mn.inputs(net, index, seed)
        check_plans(net, x, x2, "model %d, per-channel bits" % index, leave_one_out=False)


# ---------------------------------------------------------------- 4. the family: the test cannot pass by planning nothing
COUNTERS = {"resident_depthwise": "depthwise", "resident_grouped": "grouped", "resident_concats": "concat",
            "resident_upsamples": "upsample", "fused_upsamples": "upsample", "flattened_concats": "nested",
            "resident_avgpools": "avgpool", "fused_relu6s": "relu6", "resident_shuffles": "shuffle", "resident_slices": "slice",
            "resident_activations": "act"}
INTERACTIONS = ("a", "b", "c", "d", "e", "f")
LEFT = ("sum_shuffle", "sum_act", "sum_pool", "act_avgpool", "act_add", "act_two_bits", "twice", "inplace", "cat_two_grids")


def test_the_family_plans_every_feature_and_every_interaction(oracle):
    """Conditions, not measurements.  Every counter a switch adds is above zero in at least a quarter of the models that contain its
    layer type; each interaction (a) to (f) of the issue occurs at least three times; so does each class of module the planner has to
    leave alone -- counted over every plan made with everything on, the perturbed-bits arm included (readers at two bits and
    operands on two grids do not come out of a calibration: one tensor has one bit there, and a merge group one grid)."""
    runs = [checked(i) for i, _seed in FAMILY]
    for counter, kind in COUNTERS.items():
        have = [r for r in runs if r["has"].get(kind, 0) > 0]
        planned = [r for r in have if r["summary"][counter] > 0]
        assert have and 4 * len(planned) >= len(have), (counter, len(planned), len(have))
    seen = dict.fromkeys(INTERACTIONS + LEFT, 0)
    for r in runs:
        for key in seen:
            seen[key] += r["facts"][key] + (r["perturbed_facts"][key] if key in LEFT and "perturbed_facts" in r else 0)
    print("mixed family:", seen)
    assert all(seen[k] >= TIMES for k in seen), seen


# ---------------------------------------------------------------- 5. golden G22: "plain" on mixed graphs is the reference's own
def _g22_tags():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_mixed_graphs.json")) as fh:
        return sorted(json.load(fh), key=int)


@pytest.fixture(scope="module")
def g22(golden_dir):
    with open(os.path.join(golden_dir, "g22_mixed_graphs.json")) as fh:
        return json.load(fh), np.load(os.path.join(golden_dir, "g22_mixed_graphs.npz"))


def test_g22_holds_a_dozen_graphs_and_the_reference_takes_most(g22):
    ref, arrays = g22
    taken = [t for t in ref if "reference_error" not in ref[t]]
    assert len(ref) == 12 and len(taken) >= 6 and sorted(arrays.files) == sorted("logits_%s" % t for t in taken)
    assert all(ref[t]["steps"] == mn.RandomMixedNet(int(t), mn.FAMILY_SEED).steps for t in ref)


@pytest.mark.parametrize("tag", _g22_tags())
def test_g22_tables_byte_for_byte_and_logits_bit_for_bit(g22, oracle, tag):
    """The reference's graph discovery, merge groups, feat.table and both weight.tables through the oracle-backed CPU engine, and its
    ReconModel logits on the doubles: with fp32 module boundaries and with every switch on.  A graph the reference rejects (an
    assertion of its discovery) the drop-in still takes: every node has its inputs and the flow writes its tables."""
    from common.quantity import resident
    ref, arrays = g22
    index, seed = int(tag), mn.FAMILY_SEED
    got = {}
    with all_doubles.installed():
        info, (net,) = mn.calibrated(index, seed, [all_doubles.installed], record=got)
        if "reference_error" in ref[tag]:
            assert ref[tag]["reference_error"] == "AssertionError" and got["feat_table"].startswith("image ")
            assert all(v["inputs"] for v in list(got["net_info"].values())[1:])
            return
        for key in ("net_info_order", "net_info", "cared_op_layer_names", "merge_groups", "layers_num", "feat_table", "weight_table",
                    "weight_table_rewritten", "recon_layers"):
            assert got[key] == ref[tag][key], key
        x, _x2 = mn.inputs(net, index, seed)
        want = arrays["logits_%s" % tag]
        with torch.no_grad():
            np.testing.assert_array_equal(net(x).numpy(), want)
            resident.enable(net, x, **mn.ALL_SWITCHES)
            np.testing.assert_array_equal(net(x).numpy(), want, err_msg="every switch on")
