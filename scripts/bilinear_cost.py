"""What the resident int8 bilinear upsampling is worth inside a network: the resident int8-sim forward of the U-Net
(model/unet/UNet_fabu.py), resident.enable(net, x, concat=True) against resident.enable(net, x, concat=True, bilinear=True), in
one process, alternating, timed with device events.

    python scripts/bilinear_cost.py [--arms both|off|on] [--images 64] [--size 224] [--width 32] [--depth 4] [--rounds 5]
                                    [--iters 10] [--seed 0] [--out FILE]

The model is seeded, its batch norms folded (merge_bn) and it is really calibrated on the GPU on two batches of 16 seeded images
(activation_quantize, weight_quantize).  Reconstruction builds one ReconModel per arm.  Each arm's resident output is checked
against its plain forward and against the other arm's, its plan summary (with `fp32_outputs` and `resident_concats`) and what
describe().bilinear_left names are printed, then every round times `iters` forwards of each arm; a line per round, the median and
spread of each arm and the median on / off ratio are printed.  Last, fq_upsample_bilinear_i8_nhwc alone is timed at the model's
launch shapes -- back-to-back launches between device events, bytes = N H W Cpad (1 + up^2) -- next to the nearest mover at the
same shapes in the same process (fq_concat_n_i8_nhwc with one upsampled source, which moves the same bytes), with GB/s, the share
of the HBM's 8 TB/s, the ratio of the two and whether source plus output fit the 256 MiB Infinity Cache.  Runs under
scripts/ab_lib.py against another build of the library.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bilinear_cost.py --arms on --rounds 1 --iters 3

(a run of its own, no counters).
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

HBM_GBS = 8000.0
L3_BYTES = 256 << 20


def build_model(a, device):
    from common.quantity import merge_bn
    from model.unet.UNet_fabu import UNet
    torch.manual_seed(a.seed)
    model = UNet(num_classes=2, input_size=a.size, base_width=a.width, depth=a.depth)
    g = torch.Generator().manual_seed(a.seed)
    with torch.no_grad():
        for name, p in model.named_parameters():            # He-style spread for the weights; the batch norms keep gamma 1
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / max(1, p[0].numel())) ** 0.5)
            elif name.endswith("bias"):                     # (a folded bias of exactly zero has no weight bit: the quantiser takes log2 of it)
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return merge_bn(model.eval()).to(device)


def build_nets(a, arms):
    import bench
    from tools import Quantity, Reconstruction
    tmp = bench.make_workdir(1, "1,3,%d,%d" % (a.size, a.size), torch.cuda.current_device())      # cwd = its test/ directory
    g = torch.Generator(device="cuda").manual_seed(5)
    calib = [(torch.randn(16, 3, a.size, a.size, device="cuda", generator=g), None) for _ in range(2)]
    q = Quantity(build_model(a, "cuda"))
    q.activation_quantize(calib)
    q.weight_quantize()
    nets = {}
    for key in arms:
        rec = Reconstruction(build_model(a, "cuda"))
        info = rec.get_quantity_information()
        nets[key] = rec.ReconModel(info, "./workdir/recon_%s.pth" % key)
    return nets, info, tmp


def up_shapes(net, x):
    """(module name, N, H, W, C, factor) of every bilinear nn.Upsample's input, from one hooked forward."""
    rows, hooks = [], []
    for name, m in net.named_modules():
        if isinstance(m, torch.nn.Upsample) and m.mode == "bilinear":
            hooks.append(m.register_forward_hook(
                lambda mod, inp, out, name=name: rows.append((name,) + tuple(int(v) for v in (inp[0].shape[0], inp[0].shape[2], inp[0].shape[3],
                                                                                              inp[0].shape[1])) + (int(mod.scale_factor),))))
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()
    return rows


def _per_launch(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3


def time_kernels(shapes, iters=200, rounds=5):
    """Both movers at the model's shapes, alternating over `rounds`: (label, median us bilinear, median us nearest, bytes)."""
    from common.quantity import _native
    rows = []
    for (name, n, h, w, c, up) in shapes:
        cpad = _native.pad16(c)
        x = torch.randint(-128, 128, (n, h, w, cpad), dtype=torch.int8, device="cuda")
        out = torch.empty(n, up * h, up * w, cpad, dtype=torch.int8, device="cuda")
        bil, near = [], []
        for _ in range(rounds):
            bil.append(_per_launch(lambda: _native.upsample_bilinear_i8_nhwc(x, c, up, 0, False, out=out), iters))
            near.append(_per_launch(lambda: _native.concat_n_i8_nhwc([(x, c, up, False)], out=out), iters))
        rows.append(("%s [%d, %d, %d, %d] x%d" % (name, n, h, w, c, up), float(np.median(bil)), float(np.median(near)),
                     (max(bil) - min(bil)) / float(np.median(bil)), x.numel() * (1 + up * up)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from common.quantity import resident
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nets, info, tmp = build_nets(a, arms)
    say("model: UNet(base_width %d, depth %d), seed %d, really calibrated, %d images at %d x %d, arms %s"
        % (a.width, a.depth, a.seed, a.images, a.size, a.size, arms))
    say("largest fp32 tensor of the off arm: %.0f MB (a full-plane Concat of %d channels; the entry points take up to 2^31 bytes)"
        % (a.images * 2 * a.width * a.size * a.size * 4 / 1e6, 2 * a.width))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, a.size, a.size)).astype(np.float32)).cuda()
    outs = {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        assert float(plain.std()) > 0, "the output is constant"
        if key == arms[0]:
            shapes = up_shapes(net, x)
        plan = resident.enable(net, x, concat=True, bilinear=True) if key == "on" else resident.enable(net, x, concat=True)
        with torch.no_grad():
            out = net(x)
        assert torch.equal(out, plain), "resident output differs from the plain forward (%s)" % key
        outs[key] = (out, plain)
        say("%s: plan %s" % (key, dict(sorted(plan.items()))))
        say("%s: fp32_outputs %d, resident_concats %d, resident_bilinears %s"
            % (key, plan["fp32_outputs"], plan["resident_concats"], plan.get("resident_bilinears", "-")))
        for name, why in sorted(resident.describe(net).bilinear_left.items()):
            say("  left to torch: %s: %s" % (name, why))
    if len(arms) == 2:
        assert torch.equal(outs["off"][0], outs["on"][0]) and torch.equal(outs["off"][1], outs["on"][1]), "the two arms disagree"
        say("outputs: on == off == plain forward")
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
    say("fq_upsample_bilinear_i8_nhwc alone at the model's launch shapes, next to fq_concat_n_i8_nhwc with one upsampled source (back-to-back "
        "launches, device events, medians of 5 alternating rounds; bytes = N H W Cpad (1 + up^2); share of %.0f TB/s):" % (HBM_GBS / 1e3))
    for (label, us_b, us_n, spread, nbytes) in time_kernels(shapes):
        say("  %-36s bilinear %8.1f us %7.0f GB/s %5.1f %% (spread %.3f) | nearest %8.1f us %7.0f GB/s | bilinear / nearest %.3f | %8.2f MB, %s"
            % (label, us_b, nbytes / us_b / 1e3, 100.0 * nbytes / us_b / 1e3 / HBM_GBS, spread, us_n, nbytes / us_n / 1e3, us_b / us_n,
               nbytes / 1e6, "fits the Infinity Cache" if nbytes <= L3_BYTES else "larger than the Infinity Cache"))
    os.chdir(ROOT)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
