#!/usr/bin/env python3
"""Capture golden G26 (g26_requant_net.json / .npz) by running the imported reference in the build container:

    python tests/golden/make_golden_requant.py              write the golden for requant_nets.G26_SEED
    python tests/golden/make_golden_requant.py --search N   try weight seeds 0 .. N - 1 and print the ones whose calibration meets
                                                            the conditions below (nothing is written)

The net is tests/requant_nets.py's g26_net: a residual block whose ReLU(sum) is the skip of a Concat with a bilinear-upsampled
deeper branch, and a second Concat of two convolution branches, with FIXED integer-valued weights
(activation_nets.integer_weights), calibrated on integer-valued images of 16 x 16.  The reference runs with `Upsample` appended to
ALL_OP_TYPE and ALLOW_SAME_TID_OP_TYPE of its scratch tools/configs.yml, as for G25.  Recorded: the reference's graph discovery,
merge groups, feat.table, weight.table (as written and as rewritten), quantity information and the logits of its ReconModel on a
fixed input.  The fixture holds the inputs' recipe and the reference's outputs only.

Conditions of the tests that use this golden, asserted here on the reference's own run so that a regeneration cannot lose them:
  a. at least one Concat's readers quantise at another bit than the grid of one of its operands;
  b. at least one Concat has operands on two grids;
  c. one Concat operand is an Eltwise.
The grid of a convolution is its output_bit; of an Eltwise, max(0, its operands' grids) -- the reference never re-quantises a sum --;
a Concat's readers are the convolutions that list it as an input.
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


def conditions(net_info, info):
    """(a, b, c) of the module docstring as lists of Concat names, from the reference's graph and quantity information."""
    # graph nodes are named type_index in execution order; the k-th Conv2d node is the module conv<k> of requant_nets.G26Net
    module, seen = {}, {}
    for name, node in net_info.items():
        seen[node["type"]] = seen.get(node["type"], 0) + 1
        module[name] = {"Conv2d": "conv", "Linear": "fc"}.get(node["type"], node["type"]) + (str(seen[node["type"]]) if node["type"] != "Linear" else "")

    def grid(name):
        node = net_info[name]
        if node["type"] == "Eltwise":
            return max([0] + [grid(i) for i in node["inputs"]])
        return info[module[name]]["output_bit"]

    a, b, c = [], [], []
    for name, node in net_info.items():
        if node["type"] != "Concat":
            continue
        grids = [grid(i) for i in node["inputs"]]
        readers = [info[module[k]]["input_bit"] for k, v in net_info.items() if name in v["inputs"] and v["type"] == "Conv2d"]
        if any(r != g for r in readers for g in grids):
            a.append(name)
        if len(set(grids)) > 1:
            b.append(name)
        if any(net_info[i]["type"] == "Eltwise" for i in node["inputs"]):
            c.append(name)
    return a, b, c


def run(seed, cq, tl):
    import torch
    import activation_nets as an
    import requant_nets as rn
    shape = rn.G26_SHAPE
    rec = {"shape": list(shape), "seed": seed, "calib_seed": rn.G26_CALIB_SEED, "input_seed": rn.G26_INPUT_SEED}
    with _refenv.reference_workdir(input_shape="1,%d,%d,%d" % shape[1:], max_cali_img_num=2, extra_tool_cfg=_settings()) as tmp:
        torch.manual_seed(0)
        model = an.integer_weights(rn.g26_net(), base_seed=seed).eval()
        q = tl.Quantity(model)
        rec.update({"net_info": {k: v for k, v in q.net_info.items()}, "net_info_order": list(q.net_info.keys()),
                    "cared_op_layer_names": q.cared_op_layer_names, "merge_groups": q.get_merge_groups(q.net_info),
                    "layers_num": q.layers_num})
        info0 = rec["net_info"]
        assert not any(v["type"] in ("Upsample", "MaxPool2d", "ReLU") for v in info0.values()), "an Upsample is a node of the graph"
        assert sum(v["type"] == "Concat" for v in info0.values()) == 2 and sum(v["type"] == "Eltwise" for v in info0.values()) == 1
        q.activation_quantize(an.integer_batches(3, shape, rn.G26_CALIB_SEED))
        wd = os.path.join(tmp, "test", "workdir")
        rec["feat_table"] = _read(os.path.join(wd, "feat.table"))
        q.weight_quantize()
        rec["weight_table"] = _read(os.path.join(wd, "weight.table"))
        q.rewrite_weight()
        rec["weight_table_rewritten"] = _read(os.path.join(wd, "weight.table"))
        r = tl.Reconstruction(an.integer_weights(rn.g26_net(), base_seed=seed).eval())
        info = r.get_quantity_information()
        recon = r.ReconModel(info, os.path.join(wd, "recon.pth"))
        x = an.integer_input(shape, rn.G26_INPUT_SEED)
        with torch.no_grad():
            logits = recon(x).numpy()
        rec["recon_layers"] = sorted(info.keys())
        rec["quantity_information"] = {k: {kk: vv for kk, vv in v.items() if kk not in ("layer",)} for k, v in info.items()}
    return rec, x.numpy(), logits, conditions(rec["net_info"], rec["quantity_information"])


def main():
    cq, tl = _refenv.import_reference()
    import requant_nets as rn
    assert rn.Concat is cq.Concat and rn.Eltwise is cq.Eltwise
    if len(sys.argv) > 2 and sys.argv[1] == "--search":
        for seed in range(int(sys.argv[2])):
            try:
                rec, _x, logits, (a, b, c) = run(seed, cq, tl)
            except AssertionError as err:
                print("seed %d: %s" % (seed, err))
                continue
            bits = {k: (v.get("input_bit"), v.get("output_bit")) for k, v in rec["quantity_information"].items()}
            print("seed %d: a %s b %s c %s logits std %.3f bits %s" % (seed, a, b, c, float(logits.std()), bits))
        return
    rec, x, logits, (a, b, c) = run(rn.G26_SEED, cq, tl)
    print("bits:", {k: (v.get("input_bit"), v.get("output_bit")) for k, v in rec["quantity_information"].items()})
    assert a, "no Concat whose readers sit on another bit than one of its operands"
    assert b, "no Concat with operands on two grids"
    assert c, "no Concat with an Eltwise operand"
    assert float(logits.std()) > 0
    rec["conditions"] = {"reader_bit_differs": a, "two_grids": b, "eltwise_operand": c}
    with open(os.path.join(HERE, "g26_requant_net.json"), "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "g26_requant_net.npz"), x=x, logits_recon=logits)
    print("G26 written; feat.table:\n" + rec["feat_table"])
    print("merge groups:", rec["merge_groups"])
    print("conditions:", rec["conditions"])
    print("logits:", logits[0])


if __name__ == "__main__":
    main()
