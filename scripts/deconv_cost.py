"""What keeping nn.ConvTranspose2d in int8 is worth inside a network: UNet(base_width 32, depth 4,
up="deconv") (model/unet/UNet_fabu.py) with up_kernel 2 and 4 at 64 images of 224 x 224, the eager resident int8-sim forward under
resident.enable(net, x, concat=True, requant=True) against the same with deconv=True, the two arms alternating in one process, timed
with device events around `iters` forwards.

    python scripts/deconv_cost.py [--arms both|off|on] [--images 64] [--size 224] [--width 32] [--depth 4] [--rounds 5] [--iters 5]
                                  [--out FILE]
    python scripts/ab_lib.py <another libfq_hip.so> scripts/deconv_cost.py ...      the same against another build of the library

Each model gets seeded weights and is really calibrated on the GPU on two batches of seeded images; Reconstruction builds one
ReconModel per arm.  Each arm's output is checked against its plain forward and its plan summary is printed; with both arms the
outputs of the two arms must be identical (asserted).  `rounds` (at least five) timings of each arm; every round, the median and the
spread of each arm and the median on / off ratio are printed.  The `on` arm also reports what describe().deconv_left says stayed
fp32, and times the kernel alone at the launches it recorded, back to back between two device events: its time, the bytes moved
N H W Cpad + N P Q Kpad + weights, the useful MACs N H W C K R S, and their share of 8 TB/s and of the int8 MFMA peak (2.5e15 MAC/s:
twice the BF16 rate).  For the kernel == stride launches it alternates with the route that exists without the kernel:
fq_conv2d_i8_resident on the twin's 1x1 weights (W.permute(1, 2, 3, 0).reshape(4 K, C)) followed by fq_pixel_shuffle_i8_nhwc; the two
routes' bytes are asserted equal.  That route covers kernel == stride only.

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
I8_MAC_PER_S = 2.5e15
INFINITY_CACHE_BYTES = 256 << 20
BASE = dict(concat=True, requant=True)


def pad16(c):
    return (int(c) + 15) // 16 * 16


def build_model(a, up_kernel, device):
    from model.unet.UNet_fabu import UNet
    model = UNet(input_size=a.size, base_width=a.width, depth=a.depth, batch_norm=False, up="deconv", up_kernel=up_kernel)
    g = torch.Generator().manual_seed(up_kernel)
    with torch.no_grad():
        for p in model.parameters():
            fan = max(1, p[0].numel()) if p.dim() > 1 else 1
            p.copy_(torch.randn(p.shape, generator=g) * (1.0 / fan ** 0.5 if p.dim() > 1 else 0.05))
    return model.eval().to(device)


def recorded_launches(net, x):
    """[(source shape, C, K, kernel, stride, padding, output_padding, rs, relu), ...] of the fq_deconv2d_i8_resident launches of one
    forward"""
    from common.quantity import _native
    seen = []
    real = _native.deconv2d_i8_resident

    def spy(xq, wq, qbias, C, kernel, stride, padding, output_padding, rs, ob, relu, **kw):
        seen.append((tuple(int(v) for v in xq.shape), int(C), qbias.numel(), tuple(kernel), tuple(stride), tuple(padding),
                     tuple(output_padding), int(rs), bool(relu)))
        return real(xq, wq, qbias, C, kernel, stride, padding, output_padding, rs, ob, relu, **kw)

    _native.deconv2d_i8_resident = spy
    try:
        with torch.no_grad():
            net(x)
        torch.cuda.synchronize()
    finally:
        _native.deconv2d_i8_resident = real
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
    """Each distinct launch alone on random int8 operands; a kernel == stride == 2 launch alternates with the two-launch route."""
    from common.quantity import _native
    for key in sorted(set(launches)):
        shape, C, K, kernel, stride, padding, outpad, rs, relu = key
        N, H, W, cpad = shape
        g = torch.Generator(device="cuda").manual_seed(C + K)
        xq = torch.randint(-128, 128, shape, dtype=torch.int8, device="cuda", generator=g)
        w = torch.randint(-128, 128, (C, K) + kernel, device="cuda", generator=g).float()
        qb = torch.randint(-20, 21, (K,), device="cuda", generator=g).float()
        wq = _native.pack_weight_deconv(w, stride, padding)
        out = _native.deconv2d_i8_resident(xq, wq, qb, C, kernel, stride, padding, outpad, rs, 0, relu)
        nbytes = xq.numel() + out.numel() + wq.numel()
        macs = N * H * W * C * K * kernel[0] * kernel[1]
        twin = kernel == stride == (2, 2) and padding == (0, 0) and outpad == (0, 0)
        if twin:
            w1 = _native.pack_weight_krsc(w.permute(1, 2, 3, 0).reshape(4 * K, C, 1, 1).contiguous(), cpad)
            qb4 = qb.repeat_interleave(4)

            def route():
                _y, q = _native.conv2d_i8_resident(xq, w1, qb4, (1, 1), (0, 0), (1, 1), rs, 0, False, True, relu)
                return _native.pixel_shuffle_i8_nhwc(q, K, 2, 0)

            assert torch.equal(route(), out), "the two-launch route computes other bytes"
        dc, two = [], []
        for _ in range(rounds):
            dc.append(_timed(lambda: _native.deconv2d_i8_resident(xq, wq, qb, C, kernel, stride, padding, outpad, rs, 0, relu, out=out), iters))
            if twin:
                two.append(_timed(route, iters))
        md = float(np.median(dc))
        say("  kernel source %s C %d K %d kernel %s stride %s pad %s outpad %s rs %d: %d per forward, %.1f MB moved (%s the %d MB Infinity "
            "Cache), %.2f GMAC" % ("x".join(map(str, shape)), C, K, kernel, stride, padding, outpad, rs, launches.count(key), nbytes / 1e6,
                                   "fits" if nbytes <= INFINITY_CACHE_BYTES else "exceeds", INFINITY_CACHE_BYTES >> 20, macs / 1e9))
        say("    fq_deconv2d_i8_resident: median %.4f ms (min %.4f, max %.4f, spread %.3f) = %.3f TB/s, %.3f of %.0f TB/s; %.1f TMAC/s, %.4f of the "
            "int8 MFMA peak" % (md, min(dc), max(dc), (max(dc) - min(dc)) / md, nbytes / md / 1e9, nbytes / md / 1e9 / (HBM_BYTES_PER_S / 1e12),
                                HBM_BYTES_PER_S / 1e12, macs / md / 1e9, macs / (md * 1e-3) / I8_MAC_PER_S))
        if twin:
            mt = float(np.median(two))
            say("    fq_conv2d_i8_resident (1x1 to 4K) + fq_pixel_shuffle_i8_nhwc: median %.4f ms (min %.4f, max %.4f, spread %.3f); "
                "deconv / two launches: %.3f (same bytes: asserted)" % (mt, min(two), max(two), (max(two) - min(two)) / mt, md / mt))
        else:
            say("    no route without the kernel: kernel != stride")


def run_model(a, up_kernel, arms, say):
    from common.quantity import resident
    from tools import Quantity, Reconstruction
    g = torch.Generator(device="cuda").manual_seed(5)
    calib = [(torch.randn(4, 3, a.size, a.size, device="cuda", generator=g), None) for _ in range(2)]
    q = Quantity(build_model(a, up_kernel, "cuda"))
    q.activation_quantize(calib)
    q.weight_quantize()
    nets = {}
    for key in arms:
        rec = Reconstruction(build_model(a, up_kernel, "cuda"))
        nets[key] = rec.ReconModel(rec.get_quantity_information(), "./workdir/recon_k%d_%s.pth" % (up_kernel, key))
    say("resident: UNet(base_width %d, depth %d, up='deconv', up_kernel %d), %d images at %d x %d, arms %s"
        % (a.width, a.depth, up_kernel, a.images, a.size, a.size, arms))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, a.size, a.size)).astype(np.float32)).cuda()
    outs = {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        plan = resident.enable(net, x, deconv=True, **BASE) if key == "on" else resident.enable(net, x, **BASE)
        with torch.no_grad():
            out = net(x)
        assert torch.equal(out, plain), "resident output differs from the plain forward (%s)" % key
        outs[key] = out
        del plain
        say("%s: plan %s" % (key, dict(sorted(plan.items()))))
        say("%s: fp32_outputs %d" % (key, plan["fp32_outputs"]))
        if key == "on":
            left = resident.describe(net).deconv_left
            say("on: resident_deconvs %d; deconv_left: %s" % (plan["resident_deconvs"], dict(left) if left else "none"))
    if len(arms) == 2:
        assert torch.equal(outs["off"], outs["on"]), "the two arms disagree"
        say("outputs: on == off == plain forward")
    outs.clear()
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
        say("on: %d fq_deconv2d_i8_resident launches per forward" % len(launches))
        if launches:
            kernel_rate(launches, a.iters, a.rounds, say)
    for net in nets.values():
        resident.disable(net)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--kernels", default="2,4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.rounds >= 5 or a.arms != "both", "at least five timings per arm"
    import bench
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("command: python scripts/deconv_cost.py " + " ".join(sys.argv[1:]))
    tmp = bench.make_workdir(1, "1,3,%d,%d" % (a.size, a.size), torch.cuda.current_device())       # cwd = its test/ directory
    try:
        for up_kernel in (int(k) for k in a.kernels.split(",")):
            run_model(a, up_kernel, arms, say)
            torch.cuda.empty_cache()
    finally:
        os.chdir(ROOT)
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
