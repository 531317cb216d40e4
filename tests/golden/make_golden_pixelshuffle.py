#!/usr/bin/env python3
"""Capture golden G27 (g27_pixelshuffle_net.json / .npz) by running the imported reference:

    python tests/golden/make_golden_pixelshuffle.py              write the golden for pixelshuffle_nets.G27_SEED
    python tests/golden/make_golden_pixelshuffle.py --search N   try weight seeds 0 .. N - 1 and print their bits (nothing is written)

The net is tests/pixelshuffle_nets.py's g27_net: stem convolution + ReLU -> PixelUnshuffle(2) -> convolution + ReLU -> one Eltwise
residual step -> convolution to 4 C channels -> PixelShuffle(2) -> convolution, with FIXED integer-valued weights
(activation_nets.integer_weights), calibrated on integer-valued images of 16 x 16.  The reference runs with `PixelShuffle` and
`PixelUnshuffle` appended to ALL_OP_TYPE and ALLOW_SAME_TID_OP_TYPE of its scratch tools/configs.yml -- in memory, its shipped file
is not touched.  Recorded: the reference's graph discovery, merge groups, feat.table, weight.table (as written and as rewritten),
quantity information and the logits of its ReconModel on a fixed input.  The fixture holds the inputs' recipe and the reference's
outputs only.

Conditions of the tests that use this golden, asserted here on the reference's own run so that a regeneration cannot lose them:
  a. neither module is a node of the discovered graph (both are pruned one-input ops);
  b. the convolution behind each module has the input_bit of the cared layer in front of it: conv2 reads at conv1's output bit,
     conv6 at conv5's.
The weight seed is pixelshuffle_nets.G27_SEED, the first one tried; no search was needed.
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

NAMES = ["PixelShuffle", "PixelUnshuffle"]


def _read(path):
    with open(path) as fh:
        return fh.read()


def _settings():
    with open(os.path.join(_refenv.REFERENCE_ROOT, "tools", "configs.yml")) as fh:
        settings = yaml.safe_load(fh)["SETTINGS"]
    return {"ALL_OP_TYPE": list(settings["ALL_OP_TYPE"]) + NAMES,
            "ALLOW_SAME_TID_OP_TYPE": list(settings["ALLOW_SAME_TID_OP_TYPE"]) + NAMES}


def run(seed, cq, tl):
    import torch
    import activation_nets as an
    import pixelshuffle_nets as pn
    shape = pn.G27_SHAPE
    rec = {"shape": list(shape), "seed": seed, "calib_seed": pn.G27_CALIB_SEED, "input_seed": pn.G27_INPUT_SEED}
    with _refenv.reference_workdir(input_shape="1,%d,%d,%d" % shape[1:], max_cali_img_num=2, extra_tool_cfg=_settings()) as tmp:
        torch.manual_seed(0)
        model = an.integer_weights(pn.g27_net(), base_seed=seed).eval()
        q = tl.Quantity(model)
        rec.update({"net_info": {k: v for k, v in q.net_info.items()}, "net_info_order": list(q.net_info.keys()),
                    "cared_op_layer_names": q.cared_op_layer_names, "merge_groups": q.get_merge_groups(q.net_info),
                    "layers_num": q.layers_num})
        info0 = rec["net_info"]
        assert not any(v["type"] in NAMES + ["ReLU"] for v in info0.values()), "a pixel shuffle is a node of the graph"
        assert sum(v["type"] == "Conv2d" for v in info0.values()) == 6 and sum(v["type"] == "Eltwise" for v in info0.values()) == 1
        q.activation_quantize(an.integer_batches(3, shape, pn.G27_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        rec["feat_table"] = _read(os.path.join(wd, "feat.table"))
        q.weight_quantize()
        rec["weight_table"] = _read(os.path.join(wd, "weight.table"))
        q.rewrite_weight()
        rec["weight_table_rewritten"] = _read(os.path.join(wd, "weight.table"))
        r = tl.Reconstruction(an.integer_weights(pn.g27_net(), base_seed=seed).eval())
        info = r.get_quantity_information()
        recon = r.ReconModel(info, os.path.join(wd, "recon.pth"))
        x = an.integer_input(shape, pn.G27_INPUT_SEED)
        with torch.no_grad():
            logits = recon(x).numpy()
        rec["recon_layers"] = sorted(info.keys())
        rec["quantity_information"] = {k: {kk: vv for kk, vv in v.items() if kk not in ("layer",)} for k, v in info.items()}
    return rec, x.numpy(), logits


def main():
    cq, tl = _refenv.import_reference()
    import pixelshuffle_nets as pn
    assert pn.Eltwise is cq.Eltwise
    seeds = range(int(sys.argv[2])) if len(sys.argv) > 2 and sys.argv[1] == "--search" else [pn.G27_SEED]
    for seed in seeds:
        rec, x, logits = run(seed, cq, tl)
        q = rec["quantity_information"]
        bits = {k: (v.get("input_bit"), v.get("output_bit")) for k, v in q.items()}
        print("seed %d: logits std %.3f bits %s" % (seed, float(logits.std()), bits))
        ok = q["conv2"]["input_bit"] == q["conv1"]["output_bit"] and q["conv6"]["input_bit"] == q["conv5"]["output_bit"]
        if len(sys.argv) > 2:
            print("   condition b:", ok)
            continue
        assert ok, "the convolution behind a module does not read at the bit of the cared layer in front"
        assert float(logits.std()) > 0
        with open(os.path.join(HERE, "g27_pixelshuffle_net.json"), "w") as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
        np.savez_compressed(os.path.join(HERE, "g27_pixelshuffle_net.npz"), x=x, logits_recon=logits)
        print("G27 written; feat.table:\n" + rec["feat_table"])
        print("merge groups:", rec["merge_groups"])
        print("logits:", logits[0, :, 0, :4])


if __name__ == "__main__":
    main()
