#!/usr/bin/env python3
"""Capture golden G28 (g28_deconv_net.json / .npz) by running the imported reference:

    python tests/golden/make_golden_deconv.py              write the golden for deconv_nets.G28_SEED
    python tests/golden/make_golden_deconv.py --search N   try weight seeds 0 .. N - 1 and print their bits (nothing is written)

The net is tests/deconv_nets.py's G28Net: stem convolution + ReLU -> ConvTranspose2d(k=2, s=2) -> ReLU -> convolution ->
ConvTranspose2d(k=4, s=2, p=1) -> convolution, with FIXED integer-valued weights (deconv_nets.g28_weights), calibrated on
integer-valued images of 3 x 16 x 16.  The reference runs with `ConvTranspose2d` appended to CARE_OP_TYPE and ALL_OP_TYPE (and, for
the twin, `PixelShuffle` to ALL_OP_TYPE and ALLOW_SAME_TID_OP_TYPE) of its scratch tools/configs.yml -- in memory, its shipped file is
not touched.  The fixture holds the inputs' recipe and the reference's outputs only.

(a) Recorded from the reference's run of the whole net: graph discovery, merge groups, feat.table, weight.table (as written and as
    rewritten) and the quantity information.  The reference's own ReconModel leaves both up-convolutions float, so no logits of the
    whole net are recorded: the tests hold NewConvTranspose2d's logits of it against the exact integer rule instead.
(b) The twin construction.  The net that ends behind conv2 (the first up-convolution's consumer) and its twin, in which the
    kernel == stride layer is a 1x1 convolution to 4 K channels + PixelShuffle(2) (deconv_nets.g28_twin), go through the reference
    too.  Asserted here: their float outputs are equal (torch.equal) and their feat.table and both weight.tables are identical,
    byte for byte.  Recorded: the reference's own ReconModel logits of the TWIN -- what NewConvTranspose2d must reproduce bit for bit.

Conditions asserted on the reference's own run, so that a regeneration cannot lose them:
  * both up-convolutions are nodes of the discovered graph, of type ConvTranspose2d, with one input each;
  * the layers the head net shares with the whole net (conv1, up1, conv2) have the same input and weight bits in both.
The weight seed is deconv_nets.G28_SEED, the first one tried; no search was needed.
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
    return {"CARE_OP_TYPE": list(settings["CARE_OP_TYPE"]) + ["ConvTranspose2d"],
            "ALL_OP_TYPE": list(settings["ALL_OP_TYPE"]) + ["ConvTranspose2d", "PixelShuffle"],
            "ALLOW_SAME_TID_OP_TYPE": list(settings["ALLOW_SAME_TID_OP_TYPE"]) + ["PixelShuffle"]}


def calibrate(make, tl, shape, calib_seed, input_seed, recon):
    """One model through the reference's flow: (record, input, float output, ReconModel logits or None)."""
    import torch
    import activation_nets as an
    rec = {}
    with _refenv.reference_workdir(input_shape="1,%d,%d,%d" % shape[1:], max_cali_img_num=2, extra_tool_cfg=_settings()) as tmp:
        torch.manual_seed(0)
        q = tl.Quantity(make())
        rec.update({"net_info": {k: v for k, v in q.net_info.items()}, "net_info_order": list(q.net_info.keys()),
                    "cared_op_layer_names": q.cared_op_layer_names, "merge_groups": q.get_merge_groups(q.net_info),
                    "layers_num": q.layers_num})
        q.activation_quantize(an.integer_batches(3, shape, calib_seed))
        wd = os.path.join(tmp, "test", "workdir")
        rec["feat_table"] = _read(os.path.join(wd, "feat.table"))
        q.weight_quantize()
        rec["weight_table"] = _read(os.path.join(wd, "weight.table"))
        q.rewrite_weight()
        rec["weight_table_rewritten"] = _read(os.path.join(wd, "weight.table"))
        r = tl.Reconstruction(make())
        info = r.get_quantity_information()
        rec["recon_layers"] = sorted(info.keys())
        rec["quantity_information"] = {k: {kk: vv for kk, vv in v.items() if kk not in ("layer",)} for k, v in info.items()}
        x = an.integer_input(shape, input_seed)
        with torch.no_grad():
            y = make()(x).numpy()
            logits = r.ReconModel(info, os.path.join(wd, "recon.pth"))(x).numpy() if recon else None
    return rec, x.numpy(), y, logits


def run(seed, cq, tl):
    import deconv_nets as dn
    shape = dn.G28_SHAPE
    rec = {"shape": list(shape), "seed": seed, "calib_seed": dn.G28_CALIB_SEED, "input_seed": dn.G28_INPUT_SEED}
    full, x, _y, _ = calibrate(lambda: dn.g28_weights(dn.G28Net(), seed).eval(), tl, shape, dn.G28_CALIB_SEED, dn.G28_INPUT_SEED, False)
    rec.update(full)
    info = rec["net_info"]
    ups = [k for k in rec["net_info_order"] if info[k]["type"] == "ConvTranspose2d"]
    assert len(ups) == 2 and all(len(info[k]["inputs"]) == 1 for k in ups), [info[k] for k in ups]      # nodes, one input each
    assert [n for n in rec["cared_op_layer_names"] if n.startswith("up")] == ["up1", "up2"]
    for name in ("up1", "up2"):
        assert rec["quantity_information"][name]["layer_type"] == "ConvTranspose2d"
    assert sum(v["type"] == "Conv2d" for v in info.values()) == 3 and not any(v["type"] == "ReLU" for v in info.values())
    head, xh, yh, _ = calibrate(lambda: dn.g28_weights(dn.G28Net(head_only=True), seed).eval(), tl, shape, dn.G28_CALIB_SEED,
                                dn.G28_INPUT_SEED, False)

    tw, xt, yt, logits = calibrate(lambda: dn.g28_twin(seed), tl, shape, dn.G28_CALIB_SEED, dn.G28_INPUT_SEED, True)
    assert np.array_equal(xh, xt) and np.array_equal(x, xt)
    assert np.array_equal(yh, yt), "the twin's float output differs"
    for key in ("feat_table", "weight_table", "weight_table_rewritten"):
        assert head[key] == tw[key], "the twin writes another " + key
    assert tw["quantity_information"]["up1"]["layer_type"] == "Conv2d" and head["quantity_information"]["up1"]["layer_type"] == "ConvTranspose2d"
    for name in ("conv1", "up1", "conv2"):
        a, b = head["quantity_information"][name], rec["quantity_information"][name]
        assert all(a[k] == b[k] for k in ("input_bit", "weight_bit")), (name, a, b)
    rec["twin"] = {"feat_table": tw["feat_table"], "weight_table": tw["weight_table"], "weight_table_rewritten": tw["weight_table_rewritten"],
                   "quantity_information": tw["quantity_information"], "head_quantity_information": head["quantity_information"],
                   "head_net_info": head["net_info"], "head_net_info_order": head["net_info_order"],
                   "head_merge_groups": head["merge_groups"], "head_cared_op_layer_names": head["cared_op_layer_names"],
                   "head_layers_num": head["layers_num"]}
    return rec, x, yt, logits


def main():
    cq, tl = _refenv.import_reference()
    import deconv_nets as dn
    seeds = range(int(sys.argv[2])) if len(sys.argv) > 2 and sys.argv[1] == "--search" else [dn.G28_SEED]
    for seed in seeds:
        rec, x, y_float, logits = run(seed, cq, tl)
        q = rec["quantity_information"]
        bits = {k: (v.get("input_bit"), v.get("weight_bit"), v.get("output_bit")) for k, v in q.items()}
        print("seed %d: twin logits std %.3f bits (in, weight, out) %s" % (seed, float(logits.std()), bits))
        if len(sys.argv) > 2:
            continue
        assert float(logits.std()) > 0
        with open(os.path.join(HERE, "g28_deconv_net.json"), "w") as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
        np.savez_compressed(os.path.join(HERE, "g28_deconv_net.npz"), x=x, twin_float=y_float, logits_twin_recon=logits)
        print("G28 written; feat.table:\n" + rec["feat_table"])
        print("weight.table:\n" + rec["weight_table_rewritten"])
        print("merge groups:", rec["merge_groups"])


if __name__ == "__main__":
    main()
