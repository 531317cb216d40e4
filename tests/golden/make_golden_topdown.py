#!/usr/bin/env python3
"""Capture golden G24 (g24_topdown_net.json / .npz) by running the imported reference in the build container:

    python tests/golden/make_golden_topdown.py

The net is tests/topdown_nets.py's g24_net: a toy FPN -- a trunk of three stages, 1x1 laterals, two nearest-x2 top-down steps
with Eltwise (the second upsampling reads the first sum, which a 3x3 output convolution reads as well), global pool, View,
Linear -- on 3 x 16 x 16 input.
Recorded: the reference's graph discovery, merge groups, feat.table, weight.table (as written and as rewritten), its quantity
information and the logits of its ReconModel on a fixed input.  The fixture holds the inputs' recipe and the reference's outputs
only.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cases  # noqa: E402
import _refenv  # noqa: E402


def _read(path):
    with open(path) as fh:
        return fh.read()


def main():
    import torch
    cq, tl = _refenv.import_reference()                    # topdown_nets takes Eltwise / View from whichever `common` is imported: the reference's
    import topdown_nets as sn
    shape = sn.G24_SHAPE
    rec = {"shape": list(shape), "seed": sn.G24_SEED, "calib_seed": sn.G24_CALIB_SEED, "input_seed": sn.G24_INPUT_SEED}
    with _refenv.reference_workdir(input_shape="1,%d,%d,%d" % shape[1:], max_cali_img_num=2) as tmp:
        torch.manual_seed(0)
        model = cases.seed_model(sn.g24_net(), base_seed=sn.G24_SEED).eval()
        q = tl.Quantity(model)
        rec.update({"net_info": {k: v for k, v in q.net_info.items()}, "net_info_order": list(q.net_info.keys()),
                    "cared_op_layer_names": q.cared_op_layer_names, "merge_groups": q.get_merge_groups(q.net_info),
                    "layers_num": q.layers_num})
        q.activation_quantize(cases.calib_batches(3, shape, seed=sn.G24_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        rec["feat_table"] = _read(os.path.join(wd, "feat.table"))
        q.weight_quantize()
        rec["weight_table"] = _read(os.path.join(wd, "weight.table"))
        q.rewrite_weight()
        rec["weight_table_rewritten"] = _read(os.path.join(wd, "weight.table"))
        r = tl.Reconstruction(cases.seed_model(sn.g24_net(), base_seed=sn.G24_SEED).eval())
        info = r.get_quantity_information()
        recon = r.ReconModel(info, os.path.join(wd, "recon.pth"))
        x = cases.fixed_input(shape, seed=sn.G24_INPUT_SEED)
        with torch.no_grad():
            logits = recon(x).numpy()
        rec["recon_layers"] = sorted(info.keys())
        rec["quantity_information"] = {k: {kk: vv for kk, vv in v.items() if kk not in ("layer",)} for k, v in info.items()}
    with open(os.path.join(HERE, "g24_topdown_net.json"), "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "g24_topdown_net.npz"), x=x.numpy(), logits_recon=logits)
    print("G24 written; feat.table:\n" + rec["feat_table"])
    print("logits:", logits[0])


if __name__ == "__main__":
    main()
