#!/usr/bin/env python3
"""Capture golden G22 (g22_mixed_graphs.json / .npz) by running the imported reference in the build container:

    python tests/golden/make_golden_mixed.py

The graphs are the first twelve of the mixed family (tests/mixed_nets.py: RandomMixedNet(index, FAMILY_SEED)): dense, depthwise and
grouped convolutions behind nn.ReLU, nn.ReLU6 and table activations, residual steps, nested Concats with upsampled leaves,
ShuffleNet units and windowed pools in one graph.  The reference runs with the op types the drop-in's tools/configs.yml lists
beyond its shipped file (ReLU6, ChannelShuffle, Slice, the ten activation names) appended to ALL_OP_TYPE and
ALLOW_SAME_TID_OP_TYPE of its scratch tools/configs.yml -- plain settings, as goldens G18, G20 and G21 were taken.  Recorded per
graph: the reference's graph discovery, merge groups, feat.table, weight.table (as written and as rewritten), the layers of its
quantity information and the logits of its ReconModel on the family's test batch.  A graph the reference rejects is recorded with
its error and skipped by the tests, as in G11 (its value fingerprints do not survive every step the generator draws: an in-place
activation, a module called twice, a Slice that is no permutation of what discovery saw).  The fixture holds the reference's
outputs only; the inputs are the generator's, seeded.
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

GRAPHS = 12


def _read(path):
    with open(path) as fh:
        return fh.read()


def _settings():
    """ALL_OP_TYPE / ALLOW_SAME_TID_OP_TYPE of the reference's shipped file plus what the drop-in's file lists beyond it."""
    with open(os.path.join(_refenv.REFERENCE_ROOT, "tools", "configs.yml")) as fh:
        ref = yaml.safe_load(fh)["SETTINGS"]
    with open(os.path.join(ROOT, "pytorch-quantity_amd", "quantity", "tools", "configs.yml")) as fh:
        own = yaml.safe_load(fh)["SETTINGS"]
    return {key: list(ref[key]) + [n for n in own[key] if n not in ref[key]] for key in ("ALL_OP_TYPE", "ALLOW_SAME_TID_OP_TYPE")}


def main():
    import torch
    cq, tl = _refenv.import_reference()                    # mixed_nets then takes Eltwise / Concat / View from the reference
    import mixed_nets as mn
    assert mn.Concat is cq.Concat
    out, arrays = {}, {}
    for index in range(GRAPHS):
        seed = mn.FAMILY_SEED
        rec = {}
        model = mn.float_model(index, seed)
        size = model.size
        data = mn.batches(model, index, seed)
        with _refenv.reference_workdir(input_shape="1,3,%d,%d" % (size, size), max_cali_img_num=1, extra_tool_cfg=_settings()) as tmp:
            try:
                torch.manual_seed(0)
                q = tl.Quantity(model)
                rec.update({"net_info": {k: v for k, v in q.net_info.items()}, "net_info_order": list(q.net_info.keys()),
                            "cared_op_layer_names": q.cared_op_layer_names, "merge_groups": q.get_merge_groups(q.net_info),
                            "layers_num": q.layers_num})
                q.activation_quantize(data[1:])
                wd = os.path.join(tmp, "test", "workdir")
                rec["feat_table"] = _read(os.path.join(wd, "feat.table"))
                q.weight_quantize()
                rec["weight_table"] = _read(os.path.join(wd, "weight.table"))
                q.rewrite_weight()
                rec["weight_table_rewritten"] = _read(os.path.join(wd, "weight.table"))
                r = tl.Reconstruction(mn.float_model(index, seed))
                info = r.get_quantity_information()
                recon = r.ReconModel(info, os.path.join(wd, "recon.pth"))
                with torch.no_grad():
                    arrays["logits_%d" % index] = recon(data[0][0]).numpy()
                rec["recon_layers"] = sorted(info.keys())
            except Exception as e:                             # the reference rejects the graph
                rec = {"reference_error": type(e).__name__, "message": str(e)[:200]}
        rec["steps"] = list(model.steps)
        out[str(index)] = rec
        print(index, model.steps, rec.get("reference_error", "ok"), rec.get("message", ""))
    with open(os.path.join(HERE, "g22_mixed_graphs.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "g22_mixed_graphs.npz"), **arrays)
    print("G22 written: %d graphs, %d accepted" % (len(out), len(arrays)))


if __name__ == "__main__":
    main()
