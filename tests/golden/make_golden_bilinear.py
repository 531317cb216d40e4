#!/usr/bin/env python3
"""Capture golden G25 (g25_bilinear_net.json / .npz) by running the imported reference in the build container:

    python tests/golden/make_golden_bilinear.py

The net is tests/bilinear_nets.py's g25_net: a three-level encoder, two decoder levels of bilinear x2 -> Concat(skip, up) -> conv
(an nn.ReLU directly behind the first upsampling), then a bilinear x4 straight into a convolution, a pool, View and a Linear, with
FIXED integer-valued weights (activation_nets.integer_weights: the first convolution dense on the integer image, every other one
a single tap of +-1 per output channel with an integer bias, so that no engine's order of sums shows), calibrated on
integer-valued images of 16 x 16.  The reference runs with `Upsample` appended to ALL_OP_TYPE and ALLOW_SAME_TID_OP_TYPE of its
scratch tools/configs.yml (plain settings; its shipped file lists UpsamplingNearest2d only).  Recorded: the reference's graph
discovery, merge groups, feat.table, weight.table (as written and as rewritten), quantity information and the logits of its
ReconModel on a fixed input.  The fixture holds the inputs' recipe and the reference's outputs only.

Conditions of the tests that use this golden, asserted here on the reference's own run so that a regeneration cannot lose them:
every Upsample is a pruned one-input op (none is a node of the graph; the Concats' inputs are the convolutions), and the readers
of each upsampling -- through the ReLU and the Concat -- quantise at ONE bit.
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


def _settings():
    with open(os.path.join(_refenv.REFERENCE_ROOT, "tools", "configs.yml")) as fh:
        settings = yaml.safe_load(fh)["SETTINGS"]
    return {"ALL_OP_TYPE": list(settings["ALL_OP_TYPE"]) + ["Upsample"],
            "ALLOW_SAME_TID_OP_TYPE": list(settings["ALLOW_SAME_TID_OP_TYPE"]) + ["Upsample"]}


def main():
    import torch
    cq, tl = _refenv.import_reference()
    import activation_nets as an
    import bilinear_nets as bn
    assert bn.Concat is cq.Concat
    shape = bn.G25_SHAPE
    rec = {"shape": list(shape), "seed": bn.G25_SEED, "calib_seed": bn.G25_CALIB_SEED, "input_seed": bn.G25_INPUT_SEED}
    with _refenv.reference_workdir(input_shape="1,%d,%d,%d" % shape[1:], max_cali_img_num=2, extra_tool_cfg=_settings()) as tmp:
        torch.manual_seed(0)
        model = an.integer_weights(bn.g25_net(), base_seed=bn.G25_SEED).eval()
        q = tl.Quantity(model)
        rec.update({"net_info": {k: v for k, v in q.net_info.items()}, "net_info_order": list(q.net_info.keys()),
                    "cared_op_layer_names": q.cared_op_layer_names, "merge_groups": q.get_merge_groups(q.net_info),
                    "layers_num": q.layers_num})
        info0 = rec["net_info"]
        assert not any(v["type"] in ("Upsample", "MaxPool2d", "ReLU") for v in info0.values()), "an Upsample is a node of the graph"
        # (graph nodes are named type_index in execution order: the k-th Conv2d node is conv<k>, the k-th Concat node Concat<k>)
        convs = [None] + [k for k in rec["net_info_order"] if info0[k]["type"] == "Conv2d"]
        cats = [None] + [k for k in rec["net_info_order"] if info0[k]["type"] == "Concat"]
        assert len(convs) == 9 and len(cats) == 3
        assert sorted(info0[cats[1]]["inputs"]) == sorted([convs[2], convs[4]]), "Concat1 does not join conv2 and conv4 (through up1)"
        assert sorted(info0[cats[2]]["inputs"]) == sorted([convs[1], convs[5]]), "Concat2 does not join conv1 and conv5 (through up2)"
        assert info0[convs[5]]["inputs"] == [cats[1]] and info0[convs[6]]["inputs"] == [cats[2]]
        assert info0[convs[8]]["inputs"] == [convs[7]], "conv8 does not read conv7 (through up3)"
        q.activation_quantize(an.integer_batches(3, shape, bn.G25_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        rec["feat_table"] = _read(os.path.join(wd, "feat.table"))
        q.weight_quantize()
        rec["weight_table"] = _read(os.path.join(wd, "weight.table"))
        q.rewrite_weight()
        rec["weight_table_rewritten"] = _read(os.path.join(wd, "weight.table"))
        r = tl.Reconstruction(an.integer_weights(bn.g25_net(), base_seed=bn.G25_SEED).eval())
        info = r.get_quantity_information()
        recon = r.ReconModel(info, os.path.join(wd, "recon.pth"))
        x = an.integer_input(shape, bn.G25_INPUT_SEED)
        with torch.no_grad():
            logits = recon(x).numpy()
        print("bits:", {k: (v["input_bit"], v["output_bit"]) for k, v in info.items()})
        # one reader bit per upsampling: up1 -> (ReLU, Concat1) -> conv5, up2 -> Concat2 -> conv6, up3 -> conv8; a Concat's other
        # operand is written at the bit its reader reads
        assert info["conv5"]["input_bit"] == info["Concat1"]["output_bit"] == info["conv2"]["output_bit"] == info["conv4"]["output_bit"]
        assert info["conv6"]["input_bit"] == info["Concat2"]["output_bit"] == info["conv1"]["output_bit"] == info["conv5"]["output_bit"]
        assert info["conv8"]["input_bit"] == info["conv7"]["output_bit"]
        rec["recon_layers"] = sorted(info.keys())
        rec["quantity_information"] = {k: {kk: vv for kk, vv in v.items() if kk not in ("layer",)} for k, v in info.items()}
    with open(os.path.join(HERE, "g25_bilinear_net.json"), "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "g25_bilinear_net.npz"), x=x.numpy(), logits_recon=logits)
    print("G25 written; feat.table:\n" + rec["feat_table"])
    print("merge groups:", rec["merge_groups"])
    print("logits:", logits[0])


if __name__ == "__main__":
    main()
