#!/usr/bin/env python3
"""Capture golden G20 (g20_shuffle_net.json / .npz) by running the imported reference in the build container:

    python tests/golden/make_golden_shuffle.py

The net is tests/shuffle_nets.py's g20_net: a toy ShuffleNetV2 (stem, max-pool, one stride-2 unit to 20 channels, two stride-1
units with 10 + 10 halves, a 1x1, a pool, View and a Linear) with FIXED integer-valued weights, calibrated on integer-valued
images of 16 x 16.  The reference runs with `ChannelShuffle` appended to ALL_OP_TYPE and ALLOW_SAME_TID_OP_TYPE and `Slice` to
ALL_OP_TYPE of its scratch tools/configs.yml (plain settings; its shipped file lists neither, and discovery then cannot place
their outputs).  Its value fingerprint is invariant under a channel permutation, so a shuffle returns "the same tensor" to it as
a ReLU on non-negative data does.  Recorded: the reference's graph discovery, merge groups, feat.table, weight.table (as written
and as rewritten), quantity information and the logits of its ReconModel on a fixed input.  The fixture holds the inputs' recipe
and the reference's outputs only.

A condition of the tests that use this golden, asserted here on the reference's own run so that a regeneration cannot lose it:
the merge groups chain the Concats of the three consecutive units: the left half of a unit's input reaches its Concat through
pruned one-input ops only (shuffle, Slice), so the Concat of unit k is an operand of the Concat of unit k + 1 and stands in its
merge group; and the data (shuffle_nets.integer_weights: a stride-1 unit does not widen the range it reads) puts the operands of
all three Concats on one grid.  A merge group equalises the output bit of the earlier Concat with that of the later unit's
branch, not the bits of the earlier Concat's own operands: where a later branch has the wider range, its Concat joins two grids
and the integer plan leaves it in fp32 form.
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


def _settings_with_shuffle():
    with open(os.path.join(_refenv.REFERENCE_ROOT, "tools", "configs.yml")) as fh:
        settings = yaml.safe_load(fh)["SETTINGS"]
    return {"ALL_OP_TYPE": list(settings["ALL_OP_TYPE"]) + ["ChannelShuffle", "Slice"],
            "ALLOW_SAME_TID_OP_TYPE": list(settings["ALLOW_SAME_TID_OP_TYPE"]) + ["ChannelShuffle"]}


def concat_chain(merge_groups, net_info):
    """[(Concat of unit k, Concat of unit k + 1), ...]: a merge group is the operand list of one Concat; the chain holds where the
    Concat of every unit but the last is itself an operand of the next unit's Concat, i.e. stands in that one's group."""
    cats = [n for n, v in net_info.items() if v["type"] == "Concat"]
    links = []
    for a, b in zip(cats, cats[1:]):
        if a in net_info[b]["inputs"] and any(sorted(g) == sorted(net_info[b]["inputs"]) for g in merge_groups):
            links.append((a, b))
    return links


def main():
    import torch
    cq, tl = _refenv.import_reference()                    # shuffle_nets then takes Concat / View from the reference
    import shuffle_nets as sn
    assert sn.Concat is cq.Concat and not hasattr(cq, "Slice")
    shape = sn.G20_SHAPE
    rec = {"shape": list(shape), "seed": sn.G20_SEED, "calib_seed": sn.G20_CALIB_SEED, "input_seed": sn.G20_INPUT_SEED}
    with _refenv.reference_workdir(input_shape="1,%d,%d,%d" % shape[1:], max_cali_img_num=2,
                                   extra_tool_cfg=_settings_with_shuffle()) as tmp:
        torch.manual_seed(0)
        model = sn.integer_weights(sn.g20_net()).eval()
        q = tl.Quantity(model)
        rec.update({"net_info": {k: v for k, v in q.net_info.items()}, "net_info_order": list(q.net_info.keys()),
                    "cared_op_layer_names": q.cared_op_layer_names, "merge_groups": q.get_merge_groups(q.net_info),
                    "layers_num": q.layers_num})
        chain = concat_chain(rec["merge_groups"], rec["net_info"])
        assert len(chain) == 2, (chain, rec["merge_groups"])
        q.activation_quantize(sn.integer_batches(3))
        wd = os.path.join(tmp, "test", "workdir")
        rec["feat_table"] = _read(os.path.join(wd, "feat.table"))
        q.weight_quantize()
        rec["weight_table"] = _read(os.path.join(wd, "weight.table"))
        q.rewrite_weight()
        rec["weight_table_rewritten"] = _read(os.path.join(wd, "weight.table"))
        r = tl.Reconstruction(sn.integer_weights(sn.g20_net()).eval())
        info = r.get_quantity_information()
        recon = r.ReconModel(info, os.path.join(wd, "recon.pth"))
        x = sn.integer_input()
        with torch.no_grad():
            logits = recon(x).numpy()
        # ... and every operand of every Concat lies on ONE grid, so that each unit's left half (the integers of the unit before,
        # shuffled and sliced) can be joined with its right half as integers
        grids = set(info[c]["input_bit"] for c in sn.CONCATS) | set(info["units.%d.branch.2.0" % k]["output_bit"] for k in range(3))
        assert len(grids | {info["units.0.down.1.0"]["output_bit"]}) == 1, grids
        rec["recon_layers"] = sorted(info.keys())
        rec["quantity_information"] = {k: {kk: vv for kk, vv in v.items() if kk not in ("layer",)} for k, v in info.items()}
    with open(os.path.join(HERE, "g20_shuffle_net.json"), "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "g20_shuffle_net.npz"), x=x.numpy(), logits_recon=logits)
    print("G20 written; feat.table:\n" + rec["feat_table"])
    print("merge groups:", rec["merge_groups"])
    print("quantity information:", json.dumps(rec["quantity_information"], sort_keys=True))
    print("logits:", logits[0])


if __name__ == "__main__":
    main()
