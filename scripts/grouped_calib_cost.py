"""What the grouped fp32 kernel (fq_gconv_f32) is worth inside the product's headline path: the two-pass calibration
(tools.Quantity.activation_quantize) of ResNeXt-50 32x4d (model/resnext/ResNeXt_fabu.py: ResNeXt50) after merge_bn, 256
seeded images at 224 x 224 in batches of 32 that already live on the device, own_grouped off against on, alternating in one
process after Quantity.reserve_pool(), timed with the host clock around a synchronised call.

    python scripts/grouped_calib_cost.py [--arms both|off|on] [--images 256] [--batch 32] [--rounds 5] [--out FILE]

One untimed calibration per arm comes first (code load, the once-per-module checks, in the off arm the convolution library's
first-use search); then every round times one calibration of each arm; a line per round, the spread of each arm and the median
on / off ratio are printed.  The table of grouped layer shapes gives each layer's multiply-adds and algorithmic bytes per forward
-- 4 (in + out), plus 4 more per output where the kernel also writes the ReLU's result -- that a kernel trace is read against: run

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/grouped_calib_cost.py --arms on  --rounds 1
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/grouped_calib_cost.py --arms off --rounds 1

(runs of their own, no counters).  A calibration runs every layer twice per batch (pass 1: abs-max, pass 2: histogram) unless the
activation cache keeps pass 1's tensors.

`--arms off` never touches the new switch: this file copied into a checkout of the commit before the kernel gives the baseline.
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
    from model.resnext.ResNeXt_fabu import ResNeXt50
    torch.manual_seed(0)
    model = ResNeXt50(num_classes=1000, input_size=hw)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return merge_bn(model.eval()).to(device)


def grouped_shapes(model, x):
    """(name, C, K, groups, kernel, stride, H, W, Ho, Wo, a ReLU follows) of every grouped layer that is not depthwise, from one
    hooked forward."""
    rows, hooks = [], []
    mods = list(model.named_modules())
    for i, (name, m) in enumerate(mods):
        if isinstance(m, torch.nn.Conv2d) and 1 < m.groups < m.in_channels:
            relu = any(isinstance(mm, torch.nn.ReLU) for _n, mm in mods[i + 1:i + 3])       # (merge_bn leaves a stand-in for the BN)
            hooks.append(m.register_forward_hook(lambda mod, inp, out, name=name, relu=relu: rows.append(
                (name, mod.in_channels, mod.out_channels, mod.groups, mod.kernel_size[0], mod.stride[0], inp[0].shape[2], inp[0].shape[3],
                 out.shape[2], out.shape[3], relu))))
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=["both", "off", "on"], default="both")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
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
    say("model: ResNeXt50 (32 groups, 4 / 8 / 16 / 32 channels per group), calibration of %d images at 224 x 224 in %d batches of %d, arms %s"
        % (nb * a.batch, nb, a.batch, arms))
    say("grouped layers (name, C -> K in G groups, kernel, stride, HxW -> HoxWo, GMAC and algorithmic MB per %d-image forward: 4 (in + out), "
        "+ 4 out with the ReLU copy):" % (nb * a.batch))
    total, total_mac = 0.0, 0.0
    for (name, C, K, G, k, st, H, W, Ho, Wo, relu) in grouped_shapes(model, batches[0][0]):
        mb = nb * a.batch * 4.0 * (C * H * W + K * Ho * Wo * (2 if relu else 1)) / 1e6
        gmac = nb * a.batch * K * Ho * Wo * (C // G) * k * k / 1e9
        total += mb
        total_mac += gmac
        say("  %-16s %4d -> %4d G %2d (%2d per group)  %dx%d s%d  %3dx%-3d -> %3dx%-3d  %6.2f GMAC %9.2f MB%s"
            % (name, C, K, G, C // G, k, k, st, H, W, Ho, Wo, gmac, mb, "  (ReLU copy)" if relu else ""))
    say("  all grouped layers: %.1f GMAC, %.1f MB per forward = %.3f ms at 157 TFLOP/s, %.3f ms at 8 TB/s"
        % (total_mac, total, 2 * total_mac / 157.0, total / 8e3))

    def calibrate(key):
        sys.stdout = open(os.devnull, "w")
        try:
            q = Quantity(model)
            if key == "on":
                q.own_grouped = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q.activation_quantize(batches)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            sys.stdout = real_stdout
        table = open("./workdir/feat.table").read()
        return dt, q.timings, table

    tables = {}
    for key in arms:                                                                # untimed: first use of everything
        dt, _tm, tables[key] = calibrate(key)
        say("%s: first calibration of the process %.3f s" % (key, dt))
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
    os.chdir(ROOT)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
