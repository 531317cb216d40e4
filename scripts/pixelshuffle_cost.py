"""What keeping nn.PixelShuffle in int8 is worth inside a network: EDSR x2 and x4
(model/edsr/EDSR_fabu.py, 16 residual blocks of 64 features) at 16 images of 96 x 96 low resolution, the eager resident int8-sim
forward under resident.enable(net, x) against resident.enable(net, x, pixelshuffle=True), the two arms alternating in one process,
timed with device events around `iters` forwards.

    python scripts/pixelshuffle_cost.py [--arms both|off|on] [--images 16] [--size 96] [--rounds 5] [--iters 10] [--out FILE]
    python scripts/pixelshuffle_cost.py --probe [--out FILE]    the kernel alone at PROBE_LAUNCHES: shapes the two models do not launch

Each model gets seeded weights and is really calibrated on the GPU on two batches of seeded images; Reconstruction builds one
ReconModel per arm.  Each arm's output is checked against its plain forward and its plan summary is printed; with both arms the
outputs of the two arms must be identical (asserted).  `rounds` (at least five) timings of each arm; every round, the median and
the spread of each arm and the median on / off ratio are printed.  The `on` arm also reports what describe() says was left to
torch, and times the kernel alone at the launches it recorded: back to back between two device events, alternating with
fq_shuffle_i8_nhwc -- the per-byte LDS mover of DESIGN section 23 -- moving the same number of bytes (a two-group channel shuffle
of a tensor of the kernel's source size), next to the 8 TB/s of the README as a ratio, with the working set (source + output) of
each launch so that it can be held against the Infinity Cache (256 MB).

`--arms off` never names the new switch: the off arm is the plan of the commit before it.
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

HBM_BYTES_PER_S = 8.0e12
INFINITY_CACHE_BYTES = 256 << 20


# (shape of the source, C, r, inverse) of `--probe`: the inverse direction, r = 4 and the general family, each moving 75.5 MB like
# EDSR's first stage, and an RGB head
PROBE_LAUNCHES = [((16, 192, 192, 64), 64, 2, 1), ((16, 48, 48, 1024), 64, 4, 0), ((16, 192, 192, 64), 64, 4, 1),
                  ((16, 64, 64, 576), 64, 3, 0), ((16, 192, 192, 64), 64, 3, 1), ((16, 96, 96, 16), 3, 2, 0)]


def pad16(c):
    return (int(c) + 15) // 16 * 16


def build_model(scale, device):
    from model.edsr.EDSR_fabu import EDSR
    model = EDSR(scale=scale)
    g = torch.Generator().manual_seed(scale)
    with torch.no_grad():
        for p in model.parameters():
            fan = max(1, p[0].numel()) if p.dim() > 1 else 1
            p.copy_(torch.randn(p.shape, generator=g) * (1.0 / fan ** 0.5 if p.dim() > 1 else 0.05))
    return model.eval().to(device)


def recorded_launches(net, x):
    """[(shape of the source, C, r, inverse), ...] of the fq_pixel_shuffle_i8_nhwc launches of one forward"""
    from common.quantity import _native
    seen = []
    real = _native.pixel_shuffle_i8_nhwc

    def spy(x_q, C, r, inverse, out=None):
        seen.append((tuple(int(v) for v in x_q.shape), int(C), int(r), int(bool(inverse))))
        return real(x_q, C, r, inverse, out)

    _native.pixel_shuffle_i8_nhwc = spy
    try:
        with torch.no_grad():
            net(x)
        torch.cuda.synchronize()
    finally:
        _native.pixel_shuffle_i8_nhwc = real
    return seen


def _timed(fn, iters):
    fn()                                                                      # warm
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def kernel_rate(launches, iters, rounds, say):
    """Each distinct launch alone, alternating with fq_shuffle_i8_nhwc at equal bytes: a channel shuffle in two groups of a
    tensor of the source's size reads and writes as many bytes as the pixel shuffle does."""
    from common.quantity import _native
    for key in sorted(set(launches)):
        shape, C, r, inverse = key
        xq = torch.randint(-128, 128, shape, dtype=torch.int8, device="cuda")
        out = _native.pixel_shuffle_i8_nhwc(xq, C, r, inverse)
        nbytes = xq.numel() + out.numel()
        sh_out = torch.empty_like(xq)
        ps, sh = [], []
        for _ in range(rounds):
            ps.append(_timed(lambda: _native.pixel_shuffle_i8_nhwc(xq, C, r, inverse, out=out), iters))
            sh.append(_timed(lambda: _native.shuffle_i8_nhwc(xq, shape[3], 0, shape[3], 2, out=sh_out), iters))
        mp, ms = float(np.median(ps)), float(np.median(sh))
        sh_bytes = 2 * xq.numel()
        say("  kernel source %s C %d r %d inverse %d (family %d): %d per forward, %.1f MB working set (%s the %d MB Infinity Cache)"
            % ("x".join(map(str, shape)), C, r, inverse, _native.pixel_shuffle_family(C, r, inverse), launches.count(key), nbytes / 1e6,
               "fits" if nbytes <= INFINITY_CACHE_BYTES else "exceeds", INFINITY_CACHE_BYTES >> 20))
        say("    fq_pixel_shuffle_i8_nhwc: median %.4f ms (min %.4f, max %.4f) = %.3f TB/s, %.3f of %.0f TB/s"
            % (mp, min(ps), max(ps), nbytes / mp / 1e9, nbytes / mp / 1e9 / (HBM_BYTES_PER_S / 1e12), HBM_BYTES_PER_S / 1e12))
        say("    fq_shuffle_i8_nhwc, %.1f MB: median %.4f ms (min %.4f, max %.4f) = %.3f TB/s; time per byte, pixel shuffle / shuffle: %.3f"
            % (sh_bytes / 1e6, ms, min(sh), max(sh), sh_bytes / ms / 1e9, (mp / nbytes) / (ms / sh_bytes)))


def run_model(a, scale, arms, say):
    from common.quantity import resident
    from tools import Quantity, Reconstruction
    g = torch.Generator(device="cuda").manual_seed(5)
    calib = [(torch.randn(4, 3, a.size, a.size, device="cuda", generator=g), None) for _ in range(2)]
    q = Quantity(build_model(scale, "cuda"))
    q.activation_quantize(calib)
    q.weight_quantize()
    nets = {}
    for key in arms:
        rec = Reconstruction(build_model(scale, "cuda"))
        nets[key] = rec.ReconModel(rec.get_quantity_information(), "./workdir/recon_x%d_%s.pth" % (scale, key))
    say("resident: EDSR x%d, %d images at %d x %d low resolution, arms %s" % (scale, a.images, a.size, a.size, arms))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, a.size, a.size)).astype(np.float32)).cuda()
    outs = {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        plan = resident.enable(net, x, pixelshuffle=True) if key == "on" else resident.enable(net, x)
        with torch.no_grad():
            out = net(x)
        assert torch.equal(out, plain), "resident output differs from the plain forward (%s)" % key
        outs[key] = out
        say("%s: plan %s" % (key, dict(sorted(plan.items()))))
        say("%s: fp32_outputs %d" % (key, plan["fp32_outputs"]))
        if key == "on":
            left = resident.describe(net).pixelshuffle_left
            say("on: planned %d shuffles, %d unshuffles; left to torch: %s"
                % (plan["resident_pixelshuffles"], plan["resident_pixelunshuffles"], dict(left) if left else "none"))
    if len(arms) == 2:
        assert torch.equal(outs["off"], outs["on"]), "the two arms disagree"
        say("outputs: on == off == plain forward")
    per_arm = {key: [] for key in arms}
    for r in range(a.rounds):
        ms = {}
        for key in arms:
            net = nets[key]
            with torch.no_grad():
                ms[key] = _timed(lambda: net(x), a.iters)
            per_arm[key].append(ms[key])
        say("round %d: " % r + ", ".join("%s %.3f ms" % (k, ms[k]) for k in arms) + " per %d-image forward" % a.images
            + (", ratio on / off %.3f" % (ms["on"] / ms["off"]) if len(arms) == 2 else ""))
    for key in arms:
        v = per_arm[key]
        med = float(np.median(v))
        say("%s: median %.3f ms, min %.3f, max %.3f, spread (max - min) / median %.3f, %.0f images/s"
            % (key, med, min(v), max(v), (max(v) - min(v)) / med, a.images / med * 1e3))
    if len(arms) == 2:
        say("median ratio on / off: %.3f" % float(np.median([n / f for n, f in zip(per_arm["on"], per_arm["off"])])))
    if "on" in arms:
        launches = recorded_launches(nets["on"], x)
        say("on: %d fq_pixel_shuffle_i8_nhwc launches per forward" % len(launches))
        if launches:
            kernel_rate(launches, a.iters, a.rounds, say)
    for net in nets.values():
        resident.disable(net)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--probe", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.rounds >= 5 or a.arms != "both", "at least five timings per arm"
    import bench
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("command: python scripts/pixelshuffle_cost.py " + " ".join(sys.argv[1:]))
    if a.probe:
        kernel_rate(PROBE_LAUNCHES, a.iters, a.rounds, say)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    tmp = bench.make_workdir(1, "1,3,%d,%d" % (a.size, a.size), torch.cuda.current_device())       # cwd = its test/ directory
    try:
        for scale in (2, 4):
            run_model(a, scale, arms, say)
    finally:
        os.chdir(ROOT)
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
