"""Cost of per-channel weight bits in the integer simulation: the resident ResNet-50 int8-sim forward at 224 x 224, per-tensor
against per-channel weight bits, in one process, alternating, timed with device events.

    python scripts/per_channel_cost.py [--images 256] [--rounds 5] [--iters 10] [--out FILE]

The model is bench.py's (same construction, same folded weights).  It is calibrated on the GPU on two batches of 32 seeded
images (activation_quantize, weight_quantize, weight_quantize_per_channel), and Reconstruction builds the per-tensor ReconModel
from get_quantity_information() and the per-channel one from get_quantity_information_per_channel(); both go resident
(resident.enable, verified) and the per-channel resident logits are checked against its plain forward.  Each round times `iters`
forwards of each model; the line per round and the median ratio are printed.  Per-channel layers have no fq_block_tail_i8 /
_proj_i8 / fq_conv2d_i8_stem form (include/fq.h): the kernel launch counts of both models are printed so that a reader sees which
launches changed.  Run `rocprofv3 --kernel-trace --stats` around it (a run of its own) for the per-kernel times.
"""
import argparse
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pytorch-quantity_amd", "quantity"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def build_nets():
    import bench
    from tools import Quantity, Reconstruction
    tmp = bench.make_workdir(1, "1,3,224,224", torch.cuda.current_device())          # cwd = its test/ directory
    g = torch.Generator(device="cuda").manual_seed(5)
    calib = [(torch.randn(32, 3, 224, 224, device="cuda", generator=g), None) for _ in range(2)]
    q = Quantity(bench.build_model("r50", 224, "cuda"))
    q.activation_quantize(calib)
    q.weight_quantize()
    q.weight_quantize_per_channel()
    nets = {}
    for key in ("per_tensor", "per_channel"):
        rec = Reconstruction(bench.build_model("r50", 224, "cuda"))
        info = rec.get_quantity_information() if key == "per_tensor" else rec.get_quantity_information_per_channel()
        nets[key] = rec.ReconModel(info, "./workdir/recon_%s.pth" % key)
    spread = [len(set(v["weight_bit"])) for v in info.values() if isinstance(v.get("weight_bit"), list)]
    return nets, spread, tmp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from common.quantity import _native, resident
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nets, spread, tmp = build_nets()
    say("per-channel layers: %d, distinct bits per layer: min %d, median %d, max %d"
        % (len(spread), min(spread), int(np.median(spread)), max(spread)))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, 224, 224)).astype(np.float32)).cuda()
    for key in ("per_tensor", "per_channel"):
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        plan = resident.enable(net, x, verify=True)
        with torch.no_grad():
            assert torch.equal(net(x), plain), "resident logits differ from the plain forward"
        _native.conv_variant_log = {}
        with torch.no_grad():
            net(x)
        torch.cuda.synchronize()
        say("%s: resident convs %d, fused block tails %d, kernel launches per forward %s"
            % (key, plan["resident_convs"], plan.get("fused_block_tails", 0), dict(sorted(_native.conv_variant_log.items()))))
        _native.conv_variant_log = None
    ratios = []
    for r in range(a.rounds):
        ms = {}
        for key in ("per_tensor", "per_channel"):
            net = nets[key]
            with torch.no_grad():
                net(x)                                            # warm
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    net(x)
                t1.record()
            torch.cuda.synchronize()
            ms[key] = t0.elapsed_time(t1) / a.iters
        ratios.append(ms["per_channel"] / ms["per_tensor"])
        say("round %d: per-tensor %.3f ms, per-channel %.3f ms per %d-image forward, ratio %.3f"
            % (r, ms["per_tensor"], ms["per_channel"], a.images, ratios[-1]))
    say("median ratio per-channel / per-tensor: %.3f" % float(np.median(ratios)))
    os.chdir(ROOT)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
