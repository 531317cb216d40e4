#!/usr/bin/env python3
"""Capture golden G18 (g18_relu6_net.json / .npz) by running the imported reference in the build container:

    python tests/golden/make_golden_relu6.py

The net is tests/relu6_nets.py's g18_net: a small MobileNetV2 (model/mobilenetv2/MobileNetV2_fabu.py at width 0.5 on 32 x 32
images, without BatchNorm) with FIXED integer-valued weights, calibrated on integer-valued images.  The reference runs with
`ReLU6` appended to ALL_OP_TYPE and ALLOW_SAME_TID_OP_TYPE of its scratch tools/configs.yml (plain settings; its shipped file
lists ReLU only, and discovery then cannot place the output of an out-of-place ReLU6).  Recorded: the reference's graph
discovery, merge groups, feat.table, weight.table (as written and as rewritten) and the logits of its ReconModel on a fixed
input.  The fixture holds the inputs' recipe and the reference's outputs only.

The scale of the data is a condition of the tests that use this golden, asserted here on the reference's own run so that a
regeneration cannot lose it: the stem, a 1x1 expansion and a depthwise layer (relu6_nets.CLIPPED) have output_bit <= 4 and
outputs AT the clip bound as well as strictly inside it; relu6_nets.UNCLIPPED has output_bit >= 5, where the clip is no clip; no
layer in front of a ReLU6 has output_bit <= -2, where 6 would be off the output grid.
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


def _settings_with_relu6():
    with open(os.path.join(_refenv.REFERENCE_ROOT, "tools", "configs.yml")) as fh:
        settings = yaml.safe_load(fh)["SETTINGS"]
    return {key: list(settings[key]) + ["ReLU6"] for key in ("ALL_OP_TYPE", "ALLOW_SAME_TID_OP_TYPE")}


def main():
    import torch
    cq, tl = _refenv.import_reference()                    # relu6_nets loads the model file by path: Eltwise / View are the reference's
    import relu6_nets as rn
    shape = rn.G18_SHAPE
    rec = {"shape": list(shape), "seed": rn.G18_SEED, "calib_seed": rn.G18_CALIB_SEED, "input_seed": rn.G18_INPUT_SEED}
    with _refenv.reference_workdir(input_shape="1,%d,%d,%d" % shape[1:], max_cali_img_num=2,
                                   extra_tool_cfg=_settings_with_relu6()) as tmp:
        torch.manual_seed(0)
        model = rn.integer_weights(rn.g18_net()).eval()
        q = tl.Quantity(model)
        rec.update({"net_info": {k: v for k, v in q.net_info.items()}, "net_info_order": list(q.net_info.keys()),
                    "cared_op_layer_names": q.cared_op_layer_names, "merge_groups": q.get_merge_groups(q.net_info),
                    "layers_num": q.layers_num})
        q.activation_quantize(rn.integer_batches(3))
        wd = os.path.join(tmp, "test", "workdir")
        rec["feat_table"] = _read(os.path.join(wd, "feat.table"))
        q.weight_quantize()
        rec["weight_table"] = _read(os.path.join(wd, "weight.table"))
        q.rewrite_weight()
        rec["weight_table_rewritten"] = _read(os.path.join(wd, "weight.table"))
        r = tl.Reconstruction(rn.integer_weights(rn.g18_net()).eval())
        info = r.get_quantity_information()
        recon = r.ReconModel(info, os.path.join(wd, "recon.pth"))
        x = rn.integer_input()
        with torch.no_grad():
            logits = recon(x).numpy()
        rec["recon_layers"] = sorted(info.keys())
        rec["quantity_information"] = {k: {kk: vv for kk, vv in v.items() if kk not in ("layer",)} for k, v in info.items()}
        # the condition on the data
        counts = rn.bound_counts(rn.integer_weights(rn.g18_net()).eval(), x)
        ob = {k: v["output_bit"] for k, v in info.items()}
        for name in rn.CLIPPED:
            assert ob[name] <= 4 and counts[name][0] > 0 and counts[name][1] > 0, (name, ob[name], counts[name])
        for name in rn.UNCLIPPED:
            assert ob[name] >= 5, (name, ob[name])
        assert all(ob[name] >= -1 for name in counts), ob
        rec["bound_counts"] = {k: list(v) for k, v in counts.items()}
    with open(os.path.join(HERE, "g18_relu6_net.json"), "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "g18_relu6_net.npz"), x=x.numpy(), logits_recon=logits)
    print("G18 written; feat.table:\n" + rec["feat_table"])
    print("output bits:", ob)
    print("values (at the bound, inside):", counts)
    print("logits:", logits[0])


if __name__ == "__main__":
    main()
