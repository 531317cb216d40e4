#!/usr/bin/env python3
"""Capture golden G21 (g21_activation_net.json / .npz) by running the imported reference in the build container:

    python tests/golden/make_golden_activations.py

The net is tests/activation_nets.py's g21_net: conv -> LeakyReLU(0.1) -> MaxPool -> conv -> Hardswish -> Slice / Concat -> conv ->
SiLU -> nearest upsampling x2 -> Concat -> conv, then ReLU, a pool, View and a Linear, with FIXED weights (one tap per output
channel behind the first activation, so that no engine's order of sums shows), calibrated on integer-valued images of 16 x 16.
The reference runs with the eleven activation names of activation_nets.ACTIVATIONS (and ChannelShuffle / Slice, as for G20)
appended to ALL_OP_TYPE and the activation names to ALLOW_SAME_TID_OP_TYPE of its scratch tools/configs.yml (plain settings; its
shipped file lists none of them).  Every listed type is first run through the reference's discovery on a three-layer probe net
(conv -> activation -> conv) and then through its whole flow (calibration, weight quantisation, rewriting, ReconModel); the names
it takes are recorded as `accepted_names`, and those are the names the shipped tools/configs.yml lists (nn.PReLU is not among
them: it has a `weight`, which the reference's weight quantiser lists and its rewriter then finds no feature bits for).  Recorded: the
reference's graph discovery, merge groups, feat.table, weight.table (as written and as rewritten), quantity information and the
logits of its ReconModel on a fixed input.  The fixture holds the inputs' recipe and the reference's outputs only.

Conditions of the tests that use this golden, asserted here on the reference's own run so that a regeneration cannot lose them:
the activations are pruned one-input ops (none is a node of the graph), and the three convolutions that read an activation --
conv2, conv3 and conv4, the last two through Slices, Concats and the upsampling -- do so at ONE input bit per activation, and
conv3 and conv4 at the same one: the first Concat's value goes to both.
"""
import json
import os
import sys

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import _refenv  # noqa: E402


def _read(path):
    with open(path) as fh:
        return fh.read()


def _settings(names):
    with open(os.path.join(_refenv.REFERENCE_ROOT, "tools", "configs.yml")) as fh:
        settings = yaml.safe_load(fh)["SETTINGS"]
    return {"ALL_OP_TYPE": list(settings["ALL_OP_TYPE"]) + ["ChannelShuffle", "Slice"] + list(names),
            "ALLOW_SAME_TID_OP_TYPE": list(settings["ALLOW_SAME_TID_OP_TYPE"]) + ["ChannelShuffle"] + list(names)}


def main():
    import torch
    from torch import nn
    cq, tl = _refenv.import_reference()
    import activation_nets as an
    assert an.Concat is cq.Concat
    names = list(an.ACTIVATIONS)
    shape = an.G21_SHAPE
    rec = {"shape": list(shape), "seed": an.G21_SEED, "calib_seed": an.G21_CALIB_SEED, "input_seed": an.G21_INPUT_SEED,
           "activation_names": names}
    # every listed type through the reference's discovery: conv -> activation -> conv
    probes = {}
    for name, make in an.ACTIVATIONS.items():
        with _refenv.reference_workdir(input_shape="1,3,8,8", max_cali_img_num=1, extra_tool_cfg=_settings(names)) as tmp:
            torch.manual_seed(0)
            probe = nn.Sequential(nn.Conv2d(3, 4, 3, 1, 1), make(), nn.Conv2d(4, 4, 1)).eval()
            q = tl.Quantity(probe)
            probes[name] = {"layers": list(q.net_info.keys()), "inputs": {k: v["inputs"] for k, v in q.net_info.items()}}
            first, second = probes[name]["layers"]             # (two nodes: the activation is pruned)
            assert probes[name]["inputs"] == {first: [], second: [first]}, (name, probes[name])
            # ... and through the rest of the flow: calibration, weight quantisation, rewriting, ReconModel
            try:
                data = [(torch.rand(2, 3, 8, 8), torch.zeros(2, dtype=torch.long)) for _ in range(2)]
                q.activation_quantize(data)
                q.weight_quantize()
                q.rewrite_weight()
                torch.manual_seed(0)
                r = tl.Reconstruction(nn.Sequential(nn.Conv2d(3, 4, 3, 1, 1), make(), nn.Conv2d(4, 4, 1)).eval())
                r.ReconModel(r.get_quantity_information(), os.path.join(tmp, "test", "workdir", "recon.pth"))
                probes[name]["flow"] = "ok"
            except Exception as e:  # noqa: BLE001  (whatever the reference raises is the answer)
                probes[name]["flow"] = "%s: %s" % (type(e).__name__, str(e)[:200])
            print("probe", name, probes[name]["flow"])
    rec["probe_graphs"] = probes
    rec["accepted_names"] = [n for n in names if probes[n]["flow"] == "ok"]
    with _refenv.reference_workdir(input_shape="1,%d,%d,%d" % shape[1:], max_cali_img_num=2,
                                   extra_tool_cfg=_settings(names)) as tmp:
        torch.manual_seed(0)
        model = an.integer_weights(an.g21_net()).eval()
        q = tl.Quantity(model)
        rec.update({"net_info": {k: v for k, v in q.net_info.items()}, "net_info_order": list(q.net_info.keys()),
                    "cared_op_layer_names": q.cared_op_layer_names, "merge_groups": q.get_merge_groups(q.net_info),
                    "layers_num": q.layers_num})
        assert not any(v["type"] in names + ["Slice"] for v in rec["net_info"].values())
        q.activation_quantize(an.integer_batches(3, shape, an.G21_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        rec["feat_table"] = _read(os.path.join(wd, "feat.table"))
        q.weight_quantize()
        rec["weight_table"] = _read(os.path.join(wd, "weight.table"))
        q.rewrite_weight()
        rec["weight_table_rewritten"] = _read(os.path.join(wd, "weight.table"))
        r = tl.Reconstruction(an.integer_weights(an.g21_net()).eval())
        info = r.get_quantity_information()
        recon = r.ReconModel(info, os.path.join(wd, "recon.pth"))
        x = an.integer_input(shape, an.G21_INPUT_SEED)
        with torch.no_grad():
            logits = recon(x).numpy()
        print("bits:", {k: (v["input_bit"], v["output_bit"]) for k, v in info.items()})
        assert info["conv3"]["input_bit"] == info["conv4"]["input_bit"], "the first Concat's readers are on two grids"
        rec["recon_layers"] = sorted(info.keys())
        rec["quantity_information"] = {k: {kk: vv for kk, vv in v.items() if kk not in ("layer",)} for k, v in info.items()}
    with open(os.path.join(HERE, "g21_activation_net.json"), "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "g21_activation_net.npz"), x=x.numpy(), logits_recon=logits)
    print("G21 written; feat.table:\n" + rec["feat_table"])
    print("merge groups:", rec["merge_groups"])
    print("logits:", logits[0])


if __name__ == "__main__":
    main()
