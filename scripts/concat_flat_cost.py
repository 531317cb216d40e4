"""What flattening nested Concats is worth inside a network: the resident int8-sim forward of the BN-Inception-shaped model
(model/inception/Inception_fabu.py) at 224 x 224, resident.enable(net, x, concat=True, avgpool=True) against the same call with
flatten=True, in one process, alternating, timed with device events.  The twin of scripts/avgpool_cost.py, whose model, seeds
and calibration it uses.

    python scripts/concat_flat_cost.py [--arms both|off|on] [--images 256] [--rounds 5] [--iters 10] [--out FILE]

Each arm's resident logits are checked against its plain forward and the arms against each other, the plan summaries are
printed, then every round times `iters` forwards of each arm; a line per round, the median and the spread (max - min) of each arm.
The verdict line says whether the on arm's median exceeds the off arm's by more than the off arm's own spread.  For each arm the
algorithmic bytes of its Concat launches per forward are printed: int8 sources read plus int8 output written, computed from the
plan (which Concats launch, and with which leaves) and the operand shapes of one shape-only forward (concat_launch_bytes).  The
kernel's time per launch comes from a run of its own, without counters:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/concat_flat_cost.py --arms on --rounds 1 --iters 3

`--arms off` is the behaviour before the N-source kernel existed and the baseline of everything printed here.
"""
import argparse
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pytorch-quantity_amd", "quantity"), ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pad16(c):
    return (int(c) + 15) // 16 * 16


def concat_shapes(float_model, images, hw):
    """{Concat name: ((C_x, C_y), (name of the Concat that produced x or None, ... y ...), N, H, W)} from one forward of the float
    model on the meta device: shapes only, nothing is computed."""
    rows, made, keep, hooks = {}, {}, [], []
    meta = float_model.to("meta")
    for name, m in meta.named_modules():
        if type(m).__name__ == "Concat":
            def hook(mod, inp, out, name=name):
                x, y = inp[0], inp[1]
                rows[name] = ((int(x.shape[1]), int(y.shape[1])), (made.get(id(x)), made.get(id(y))), int(out.shape[0]), int(out.shape[2]),
                              int(out.shape[3]))
                made[id(out)] = name
                keep.append(out)                                         # (ids are not reused while the tensor lives)
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        meta(torch.empty(images, 3, hw, hw, device="meta"))
    for h in hooks:
        h.remove()
    return rows


def concat_launch_bytes(plans, shapes):
    """[(Concat name, [leaf channel counts], bytes)] of the Concat launches of one forward under the plan `plans`
    (resident.describe): a planned Concat that is not deferred launches once, with the leaves of its deferred operands in place
    of them; bytes = (sum of pad16(C_leaf) + pad16(sum C)) * N * H * W.  (No upsampled operand in this model.)"""
    def leaves(name):
        (cx, cy), (px, py), _n, _h, _w = shapes[name]
        out = []
        for c, inner in ((cx, px), (cy, py)):
            out += leaves(inner) if inner is not None and inner in plans and plans[inner].defer else [c]
        return out

    rows = []
    for name in shapes:
        if name in plans and not plans[name].defer:
            lv = leaves(name)
            _c, _p, n, h, w = shapes[name]
            rows.append((name, lv, (sum(pad16(c) for c in lv) + pad16(sum(lv))) * n * h * w))
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
    import avgpool_cost
    from common.quantity import resident
    arms = ["off", "on"] if a.arms == "both" else [a.arms]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nets, _info, tmp = avgpool_cost.build_nets(arms)
    shapes = concat_shapes(avgpool_cost.build_model(224, "cpu"), a.images, 224)
    say("model: BN-Inception shape, %d images at 224 x 224, arms %s" % (a.images, arms))
    x = torch.from_numpy(np.random.default_rng(99).standard_normal((a.images, 3, 224, 224)).astype(np.float32)).cuda()
    logits, nbytes = {}, {}
    for key in arms:
        net = nets[key]
        with torch.no_grad():
            plain = net(x)
        plan = resident.enable(net, x, concat=True, avgpool=True, flatten=(key == "on"))
        with torch.no_grad():
            out = net(x)
        assert torch.equal(out, plain), "resident logits differ from the plain forward (%s)" % key
        logits[key] = (out, plain)
        say("%s: plan %s" % (key, dict(sorted(plan.items()))))
        rows = concat_launch_bytes(resident.describe(net), shapes)
        nbytes[key] = sum(b for _n, _l, b in rows)
        say("%s: %d Concat launches per forward, %.2f MB (int8 sources read + int8 output written, %d images):"
            % (key, len(rows), nbytes[key] / 1e6, a.images))
        for name, lv, b in rows:
            say("  %-22s leaves %-18s %8.2f MB" % (name, lv, b / 1e6))
    if len(arms) == 2:
        assert torch.equal(logits["off"][0], logits["on"][0]) and torch.equal(logits["off"][1], logits["on"][1]), "the two arms disagree"
        say("logits: on == off == plain forward")
        say("Concat bytes per forward: off %.2f MB, on %.2f MB, ratio %.3f" % (nbytes["off"] / 1e6, nbytes["on"] / 1e6,
                                                                             nbytes["on"] / nbytes["off"]))
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
        say("round %d: " % r + ", ".join("%s %.3f ms" % (k, ms[k]) for k in arms) + " per %d-image forward" % a.images)
    med = {}
    for key in arms:
        v = per_arm[key]
        med[key] = float(np.median(v))
        say("%s: median %.3f ms, min %.3f, max %.3f, spread (max - min) %.3f ms, %.0f images/s"
            % (key, med[key], min(v), max(v), max(v) - min(v), a.images / med[key] * 1e3))
    if len(arms) == 2:
        spread = max(per_arm["off"]) - min(per_arm["off"])
        say("on - off (medians) %.3f ms against the off arm's spread %.3f ms: %s"
            % (med["on"] - med["off"], spread, "within the bound" if med["on"] <= med["off"] + spread else "EXCEEDS the bound"))
    os.chdir(ROOT)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
