"""What the int8 Concat kernel is worth inside a network: the resident int8-sim forward of the SqueezeNet-1.1-shaped model
(model/squeezenet/SqueezeNet_fabu.py) at 224 x 224, resident.enable(net, x) against resident.enable(net, x, concat=True), in one
process, alternating, timed with device events.

    python scripts/concat_cost.py [--arms both|off|on] [--images 256] [--rounds 5] [--iters 10] [--out FILE]

The model is seeded and calibrated on the GPU on two batches of 32 seeded images (activation_quantize, weight_quantize: the two
expand layers of every Fire module share one bit through the Concat merge group); Reconstruction builds one ReconModel per arm.
Each arm's resident logits are checked against its plain forward, its plan summary is printed, then every round times `iters`
forwards of each arm; a line per round, the spread of each arm and the median on / off ratio are printed.  The table of Concat
shapes gives the algorithmic bytes of each launch (int8 sources read + int8 output written) that a kernel trace is read against:

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/concat_cost.py --arms on --rounds 1 --iters 3

(a run of its own, no counters).  `--arms off` calls resident.enable(net, x) without the new argument: the behaviour before
the kernel existed, and the baseline of every ratio printed here.
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


def build_model(hw, device):
    from model.squeezenet.SqueezeNet_fabu import SqueezeNet
    torch.manual_seed(0)
    model = SqueezeNet(num_classes=1000, input_size=hw)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in model.parameters():                    # a spread that keeps every layer's activations alive through 26 layers
            fan = max(1, p[0].numel()) if p.dim() > 1 else 1
            p.copy_(torch.randn(p.shape, generator=g) * ((2.0 / fan) ** 0.5 if p.dim() > 1 else 0.05))
    return model.eval().to(device)


def build_nets(arms):
    import bench
    from tools import Quantity, Reconstruction
    tmp = bench.make_workdir(1, "1,3,224,224", torch.cuda.current_device())          # cwd = its test/ directory
    g = torch.Generator(device="cuda").manual_seed(5)
    calib = [(torch.randn(32, 3, 224, 224, device="cuda", generator=g), None) for _ in range(2)]
    q = Quantity(build_model(224, "cuda"))
    q.activation_quantize(calib)
    q.weight_quantize()
    nets = {}
    for key in arms:
        rec = Reconstruction(build_model(224, "cuda"))
        info = rec.get_quantity_information()
        nets[key] = rec.ReconModel(info, "./workdir/recon_%s.pth" % key)
    return nets, info, tmp


def concat_shapes(net, images):
    """(name, C0, C1, H, W, algorithmic bytes) of every Concat, from one hooked forward."""
    rows, hooks = [], []
    for name, m in net.named_modules():
        if type(m).__name__ == "Concat":
            def hook(mod, inp, out, name=name):
                n, _c, H, W = out.shape
                c0, c1 = inp[0].shape[1], inp[1].shape[1]
                pad = lambda c: (c + 15) // 16 * 16
                rows.append((name, c0, c1, H, W, n * H * W * (pad(c0) + pad(c1) + pad(c0 + c1))))
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        net(torch.zeros(images, 3, 224, 224, device="cuda"))
    for h in hooks:
        h.remove()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from common.quantity import _native, resident
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nets, info, tmp = build_nets(arms)
    say("model: SqueezeNet 1.1 shape, %d images at 224 x 224, arms %s" % (a.images, arms))
    fires = sorted(n[:-len(".Concat")] for n in info if n.endswith(".Concat"))
    shared = [f for f in fires if info[f + ".expand1x1"]["output_bit"] == info[f + ".expand3x3"]["output_bit"]]
    say("Fire modules whose two expand layers share one output bit (the Concat merge group): %d of %d" % (len(shared), len(fires)))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, 224, 224)).astype(np.float32)).cuda()
    logits = {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        if key == arms[0]:
            say("Concat launches (name, C0 + C1, plane, int8 sources read + int8 output written in MB for %d images):" % a.images)
            total = 0
            for (name, c0, c1, H, W, nbytes) in concat_shapes(net, a.images):
                say("  %-22s %4d + %-4d %3dx%-3d %8.2f MB" % (name, c0, c1, H, W, nbytes / 1e6))
                total += nbytes
            say("  all Concats of one forward: %.2f MB" % (total / 1e6))
        plan = resident.enable(net, x, concat=True) if key == "on" else resident.enable(net, x)
        with torch.no_grad():
            out = net(x)
        assert torch.equal(out, plain), "resident logits differ from the plain forward (%s)" % key
        logits[key] = out
        _native.conv_variant_log = {}
        with torch.no_grad():
            net(x)
        torch.cuda.synchronize()
        say("%s: plan %s" % (key, dict(sorted(plan.items()))))
        say("%s: integer-kernel launches per forward %s" % (key, dict(sorted(_native.conv_variant_log.items()))))
        _native.conv_variant_log = None
    if len(arms) == 2:
        assert torch.equal(logits["off"], logits["on"]), "the two arms disagree"
        say("logits: on == off == plain forward")
    per_arm = {key: [] for key in arms}
    for r in range(a.rounds):
        ms = {}
        for key in arms:
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
            per_arm[key].append(ms[key])
        say("round %d: " % r + ", ".join("%s %.3f ms" % (k, ms[k]) for k in arms) + " per %d-image forward" % a.images
            + (", ratio on / off %.3f" % (ms["on"] / ms["off"]) if len(arms) == 2 else ""))
    for key in arms:
        v = per_arm[key]
        say("%s: median %.3f ms, min %.3f, max %.3f, spread (max - min) / median %.3f, %.0f images/s"
            % (key, float(np.median(v)), min(v), max(v), (max(v) - min(v)) / float(np.median(v)), a.images / float(np.median(v)) * 1e3))
    if len(arms) == 2:
        say("median ratio on / off: %.3f" % float(np.median([n / f for n, f in zip(per_arm["on"], per_arm["off"])])))
    os.chdir(ROOT)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
