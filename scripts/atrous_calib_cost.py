"""What the atrous depthwise fp32 kernel (fq_dwconv_dil_f32) is worth inside the two-pass calibration
(tools.Quantity.activation_quantize) of DeepLabV3+ (model/deeplab/DeepLabV3Plus_fabu.py, output stride 16) after merge_bn: 64
seeded images at 224 x 224 in batches of 16 that already live on the device.  Both arms run with own_depthwise and fuse_relu6
on; own_atrous is off in one and on in the other.  The arms alternate in one process after Quantity.reserve_pool(), timed with
the host clock around a synchronised call.

    python scripts/atrous_calib_cost.py [--arms both|off|on] [--images 64] [--batch 16] [--rounds 5] [--out FILE]

One untimed calibration per arm comes first; then every round times one calibration of each arm; a line per round, the spread
of each arm and the median on / off ratio are printed, and the tables of the arms are compared.  Then, per distinct launch shape
of the seven atrous layers, the kernel alone (abs-max and the layer's ReLU / ReLU6 copy in its epilogue) against what it
replaces -- the library's grouped convolution, the bias-add producer with the abs-max, and torch's ReLU6 where the layer has one
-- in device-event time over 50 launches each, five alternating repeats; the algorithmic 8 bytes per output (4 in, 4 out, the
activation copy not counted) over the kernel's time is its share of 8 TB/s.  Last, the first calibration of a FRESH child
process in each arm (`--first`), where the off arm meets the convolution library's first-use solver search.
"""
import argparse
import os
import shutil
import subprocess
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
    from model.deeplab.DeepLabV3Plus_fabu import DeepLabV3Plus
    torch.manual_seed(0)
    model = DeepLabV3Plus(num_classes=21, output_stride=16, input_size=hw)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return merge_bn(model.eval()).to(device)


def atrous_shapes(model, x):
    """(name, C, kernel, dilation, H, W, the activation class behind it) of every atrous depthwise layer, from one hooked forward."""
    rows, hooks = [], []
    mods = list(model.named_modules())
    for i, (name, m) in enumerate(mods):
        if isinstance(m, torch.nn.Conv2d) and m.groups > 1 and m.groups == m.in_channels == m.out_channels and m.dilation[0] > 1:
            act = next((type(mm) for _n, mm in mods[i + 1:i + 3] if isinstance(mm, (torch.nn.ReLU, torch.nn.ReLU6))), None)
            hooks.append(m.register_forward_hook(lambda mod, inp, out, name=name, act=act: rows.append(
                (name, mod.out_channels, mod.kernel_size[0], mod.dilation[0], inp[0].shape[2], inp[0].shape[3], act))))
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    return rows


def time_shapes(shapes, n, say):
    """Per distinct (C, k, d, H, W, activation): the kernel alone against the launches it replaces, microseconds per call."""
    from common.quantity import _native
    g = torch.Generator().manual_seed(5)
    for (C, k, d, H, W, act) in shapes:
        x = torch.randn(n, C, H, W, generator=g).cuda()
        w = (torch.randn(C, 1, k, k, generator=g) / k).cuda()
        b = torch.randn(C, generator=g).cuda()
        mx, r = torch.zeros(1, device="cuda"), torch.empty(n, C, H, W, device="cuda")
        cap = dict(act=6.0) if act is torch.nn.ReLU6 else {}

        def own():
            _native.dwconv_dil_f32(x, w, b, (k, k), d, d, max_dev=mx, row=0, relu_out=r, **cap)

        def library():
            y = torch.nn.functional.conv2d(x, w, None, padding=d, dilation=d, groups=C)
            if act is torch.nn.ReLU6:
                _native.bias_add_absmax(y, b, mx, 0)
                torch.nn.functional.relu6(y)
            else:
                _native.bias_add_absmax(y, b, mx, 0, relu_out=r)

        def timed(fn, reps=50):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) * 1e3 / reps
        for fn in (own, library):                                                   # warm-up: code load, the library's search
            timed(fn, 5)
        to, tl = [], []
        for _ in range(5):
            to.append(timed(own))
            tl.append(timed(library))
        mo, ml = float(np.median(to)), float(np.median(tl))
        gb = 8.0 * n * C * H * W / 1e9
        say("  C %4d %dx%d d %2d %3dx%-3d %-5s kernel %8.1f us [%.1f .. %.1f]  replaced %8.1f us [%.1f .. %.1f]  ratio %.3f  "
            "%.2f GB at 8 B/output = %.1f%% of 8 TB/s"
            % (C, k, k, d, H, W, act.__name__ if act else "-", mo, min(to), max(to), ml, min(tl), max(tl), mo / ml, gb,
               100.0 * gb / (mo * 1e-6) / 8e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--first", action="store_true", help="one calibration of each arm given, timed, nothing else (the child process)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    import bench
    from tools import Quantity
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    nb = a.images // a.batch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    real_stdout = sys.stdout
    tmp = bench.make_workdir(nb - 1, "1,3,224,224", torch.cuda.current_device())     # cwd = its test/ directory
    sys.stdout = open(os.devnull, "w")                                              # the drop-in prints like the reference does
    model = build_model(224, "cuda")
    sys.stdout = real_stdout
    rng = np.random.default_rng(99)
    batches = [(torch.from_numpy(rng.standard_normal((a.batch, 3, 224, 224)).astype(np.float32)).cuda(),
                torch.zeros(a.batch, dtype=torch.long)) for _ in range(nb)]

    def calibrate(key):
        sys.stdout = open(os.devnull, "w")
        try:
            q = Quantity(model)
            q.own_depthwise, q.fuse_relu6 = True, True
            if key == "on":
                q.own_atrous = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q.activation_quantize(batches)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            sys.stdout = real_stdout
        return dt, q.timings, open("./workdir/feat.table").read()

    if a.first:
        for key in arms:
            say("FIRST %s %.3f" % (key, calibrate(key)[0]))
        os.chdir(ROOT)
        shutil.rmtree(tmp, ignore_errors=True)
        return
    say("model: DeepLabV3+ output stride 16, calibration of %d images at 224 x 224 in %d batches of %d, own_depthwise and fuse_relu6 "
        "on, own_atrous arms %s" % (nb * a.batch, nb, a.batch, arms))
    layers = atrous_shapes(model, batches[0][0])
    for (name, C, k, d, H, W, act) in layers:
        say("  %-28s C %4d  %dx%d d %2d  %3dx%-3d  %s" % (name, C, k, k, d, H, W, act.__name__ if act else "-"))
    tables = {}
    for key in arms:                                                                # untimed: first use of everything
        dt, _tm, tables[key] = calibrate(key)
        say("%s: first calibration of this process %.3f s" % (key, dt))
    Quantity.reserve_pool()
    for key in arms:
        dt, tm, table = calibrate(key)
        assert table == tables[key], "feat.table of arm %s changed from one calibration to the next" % key
        say("%s: own_conv1x1_launches %s, fused_hist_launches %s, cached_batches %s, pass1 %.3f s, pass2 %.3f s"
            % (key, tm.get("own_conv1x1_launches"), tm.get("fused_hist_launches"), tm.get("cached_batches"), tm.get("pass1_s"), tm.get("pass2_s")))
    if len(arms) == 2:
        ra, rb = tables["off"].splitlines(), tables["on"].splitlines()
        say("feat.table rows that differ between the arms: %d of %d" % (sum(u != v for u, v in zip(ra, rb)), len(ra)))
    per_arm = {key: [] for key in arms}
    for r in range(a.rounds):
        s = {}
        for key in arms:
            s[key], _tm, _t = calibrate(key)
            per_arm[key].append(s[key])
        say("round %d: " % r + ", ".join("%s %.4f s" % (k, s[k]) for k in arms) + " per %d-image calibration" % (nb * a.batch)
            + (", ratio on / off %.3f" % (s["on"] / s["off"]) if len(arms) == 2 else ""))
    for key in arms:
        v = per_arm[key]
        say("%s: median %.4f s, min %.4f, max %.4f, spread (max - min) / median %.3f, %.0f images/s"
            % (key, float(np.median(v)), min(v), max(v), (max(v) - min(v)) / float(np.median(v)), nb * a.batch / float(np.median(v))))
    if len(arms) == 2:
        say("median ratio on / off: %.3f" % float(np.median([n / f for n, f in zip(per_arm["on"], per_arm["off"])])))
    say("per launch shape at N = %d, microseconds per call, median [min .. max] of 5 x 50 launches:" % a.batch)
    time_shapes(sorted(set(row[1:] for row in layers), key=lambda t: (t[2], t[0])), a.batch, say)
    os.chdir(ROOT)
    shutil.rmtree(tmp, ignore_errors=True)
    for key in arms:                                                                # a fresh process per arm: its first calibration
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--first", "--arms", key, "--images", str(a.images),
                              "--batch", str(a.batch)], capture_output=True, text=True, timeout=600)
        first = [ln for ln in out.stdout.splitlines() if ln.startswith("FIRST ")]
        say("fresh process, arm %s: first calibration %s s" % (key, first[0].split()[2] if first else "failed: " + out.stderr[-300:]))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
