"""What fusing nn.ReLU6 is worth inside a network: MobileNetV2 (model/mobilenetv2/MobileNetV2_fabu.py) at
256 images of 224 x 224, two measurements in one process, the arms of each alternating:

  resident     the resident int8-sim forward, resident.enable(net, x, depthwise=True) against (..., depthwise=True, relu6=True),
               timed with device events around `iters` forwards;
  calibration  the two-pass calibration (tools.Quantity.activation_quantize) with own_depthwise, fuse_relu6 off against on, after
               Quantity.reserve_pool(), timed with the host clock around a synchronised call.

    python scripts/relu6_cost.py [--arms both|off|on] [--part both|resident|calibration] [--images 256] [--batch 32]
                                 [--rounds 5] [--iters 10] [--out FILE]

The model gets seeded BatchNorm statistics (as bench.py gives ResNet-50), is folded (merge_bn) and calibrated on the GPU on two
batches of 32 seeded images; Reconstruction builds one ReconModel per arm.  Each resident arm's logits are checked against its
plain forward and its plan summary and kernel launch counts are printed; with both arms the logits and the feat.tables of the two
arms must be identical (asserted).  Every measurement takes `rounds` (at least five) timings of each arm and prints each round,
the median and the spread of each arm, and the median on / off ratio.

`--arms off` never names the new switches: this file and model/mobilenetv2/ (plain torch modules) copied into a checkout of the
commit before them, with ReLU6 added to the two lists of tools/configs.yml, give the baseline.
"""
import argparse
import os
import shutil
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pytorch-quantity_amd", "quantity"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def build_model(hw, device):
    from common.quantity import merge_bn
    from model.mobilenetv2.MobileNetV2_fabu import MobileNetV2
    torch.manual_seed(0)
    model = MobileNetV2(num_classes=1000, input_size=hw)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return merge_bn(model.eval()).to(device)


def summarise(say, per_arm, arms, unit, fmt, images):
    for key in arms:
        v = per_arm[key]
        med = float(np.median(v))
        say(("%s: median " + fmt + " %s, min " + fmt + ", max " + fmt + ", spread (max - min) / median %.3f, %.0f images/s")
            % (key, med, unit, min(v), max(v), (max(v) - min(v)) / med, images / med * (1e3 if unit == "ms" else 1.0)))
    if len(arms) == 2:
        say("median ratio on / off: %.3f" % float(np.median([n / f for n, f in zip(per_arm["on"], per_arm["off"])])))


def resident_part(a, arms, say):
    from common.quantity import _native, resident
    from tools import Quantity, Reconstruction
    g = torch.Generator(device="cuda").manual_seed(5)
    calib = [(torch.randn(32, 3, 224, 224, device="cuda", generator=g), None) for _ in range(2)]
    q = Quantity(build_model(224, "cuda"))
    q.activation_quantize(calib)
    q.weight_quantize()
    nets = {}
    for key in arms:
        rec = Reconstruction(build_model(224, "cuda"))
        nets[key] = rec.ReconModel(rec.get_quantity_information(), "./workdir/recon_%s.pth" % key)
    say("resident: MobileNetV2, %d images at 224 x 224, arms %s" % (a.images, arms))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, 224, 224)).astype(np.float32)).cuda()
    logits = {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        plan = resident.enable(net, x, depthwise=True, relu6=True) if key == "on" else resident.enable(net, x, depthwise=True)
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
        if key == "on":
            left = resident.describe(net).relu6_left
            say("on: ReLU6 modules left to torch: %s" % (dict(left) if left else "none"))
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
    summarise(say, per_arm, arms, "ms", "%.3f", a.images)


def calibration_part(a, arms, say):
    from tools import Quantity
    nb = a.images // a.batch
    real_stdout = sys.stdout
    sys.stdout = open(os.devnull, "w")                            # the drop-in prints like the reference does
    model = build_model(224, "cuda")
    sys.stdout = real_stdout
    rng = np.random.default_rng(99)
    batches = [(torch.from_numpy(rng.standard_normal((a.batch, 3, 224, 224)).astype(np.float32)).cuda(),
                torch.zeros(a.batch, dtype=torch.long)) for _ in range(nb)]
    say("calibration: MobileNetV2, %d images at 224 x 224 in %d batches of %d, own_depthwise on, arms %s (fuse_relu6)"
        % (nb * a.batch, nb, a.batch, arms))

    def calibrate(key):
        sys.stdout = open(os.devnull, "w")
        try:
            q = Quantity(model)
            q.own_depthwise = True
            if key == "on":
                q.fuse_relu6 = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q.activation_quantize(batches)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            sys.stdout = real_stdout
        return dt, q.timings, open("./workdir/feat.table").read()

    tables = {}
    for key in arms:                                              # untimed: first use of everything
        dt, _tm, tables[key] = calibrate(key)
        say("%s: first calibration of the process %.3f s" % (key, dt))
    Quantity.reserve_pool()
    for key in arms:
        dt, tm, table = calibrate(key)
        assert table == tables[key], "feat.table of arm %s changed from one calibration to the next" % key
        say("%s: own_conv1x1_launches %s, fused_hist_launches %s, fused_relus %s, launches_without_own_output %s, pass1 %.3f s, pass2 %.3f s"
            % (key, tm.get("own_conv1x1_launches"), tm.get("fused_hist_launches"), tm.get("fused_relus"),
               tm.get("launches_without_own_output"), tm.get("pass1_s"), tm.get("pass2_s")))
    if len(arms) == 2:
        assert tables["off"] == tables["on"], "the feat.tables of the two arms differ"
        say("feat.table: on == off (%d rows)" % len(tables["on"].splitlines()))
    per_arm = {key: [] for key in arms}
    for r in range(a.rounds):
        s = {}
        for key in arms:
            s[key], _tm, table = calibrate(key)
            assert table == tables[key]
            per_arm[key].append(s[key])
        say("round %d: " % r + ", ".join("%s %.4f s" % (k, s[k]) for k in arms) + " per %d-image calibration" % (nb * a.batch)
            + (", ratio on / off %.3f" % (s["on"] / s["off"]) if len(arms) == 2 else ""))
    summarise(say, per_arm, arms, "s", "%.4f", nb * a.batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--part", choices=["both", "resident", "calibration"], default="both")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
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

    say("command: python scripts/relu6_cost.py " + " ".join(sys.argv[1:]))
    parts = [(resident_part, 1)] if a.part != "calibration" else []
    parts += [(calibration_part, a.images // a.batch - 1)] if a.part != "resident" else []
    for part, last_batch in parts:                                # (a scratch tree each: MAX_CALI_IMG_NUM is a setting of the tree)
        tmp = bench.make_workdir(last_batch, "1,3,224,224", torch.cuda.current_device())   # cwd = its test/ directory
        try:
            part(a, arms, say)
        finally:
            os.chdir(ROOT)
            shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
