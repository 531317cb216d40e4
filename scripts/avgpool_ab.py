"""Time the two windowed average-pool entry points of two builds of libfq_hip.so against each other on one GPU.

    python scripts/avgpool_ab.py OLD.so NEW.so [--rounds 7] [--out FILE]

The method of scripts/concat_ab.py: one process loads both libraries with ctypes and calls fq_avgpool_i8_nhwc /
fq_avgpool_i16_nhwc directly (the C ABI is the same in both).  Per shape: the outputs of the two libraries are compared for
equality, every arm is warmed up, then `rounds` rounds of old, new, old again, each timed with device events around enough
launches that a round lasts about 30 ms; the launches rotate over several buffer sets so that the working set is larger than the
last-level cache.  Prints median / min / max / spread per arm, algorithmic bytes (source read + output written) and TB/s from the
median, and the rule: new median <= old median + the old arm's spread (max - min over its rounds).  Exit status 1 when a shape
misses the rule or an output differs.  The shapes are read from the models themselves, at 256 images: every windowed nn.AvgPool2d
that scripts/avgpool_cost.py's model launches (model/inception/Inception_fabu.py at 224 x 224, int8 sources) and every one that
scripts/resnetd_cost.py's does (ResNet-50-D, the int16 shortcut sums), through those scripts' own build_model and pool_shapes."""
import argparse
import ctypes
import statistics
import sys

import torch

IMAGES = 256


def shapes():
    """(name, entry, element dtype, N, H, W, C, (kh, kw, sh, sw, ph, pw)) of every windowed pool of the two cost scripts' models"""
    import avgpool_cost
    import resnetd_cost
    pair = lambda v: (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))
    out = []
    for mod, entry, dtype in ((avgpool_cost, "fq_avgpool_i8_nhwc", torch.int8), (resnetd_cost, "fq_avgpool_i16_nhwc", torch.int16)):
        net = mod.build_model(224, "cuda")
        for (name, c, k, s, p, H, W, _P, _Q, _bytes) in mod.pool_shapes(net, 2):
            win = pair(k) + pair(s) + pair(p)
            out.append(("%s %dx%d x %d, %dx%d / %d,%d / %d,%d" % ((name, H, W, c) + win), entry, dtype, IMAGES, H, W, c, win))
        del net
    torch.cuda.empty_cache()
    return out


def pad16(c):
    return (c + 15) // 16 * 16


def load(path):
    L = ctypes.CDLL(path)
    ci, vp = ctypes.c_int, ctypes.c_void_p
    for entry in ("fq_avgpool_i8_nhwc", "fq_avgpool_i16_nhwc"):
        getattr(L, entry).restype = ci
        getattr(L, entry).argtypes = [vp, vp] + [ci] * 14 + [vp]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    libs = {"old": load(a.old), "new": load(a.new)}
    lines, failed = [], False

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("average-pool entry points, old / new = the two libraries given, %s, %d rounds of old / new / old again" % (torch.cuda.get_device_name(0), a.rounds))
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, entry, dtype, N, H, W, C, (kh, kw, sh, sw, ph, pw) in shapes():
        cpad = pad16(C)
        P, Q = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        esize = 1 if dtype == torch.int8 else 2
        lim = 128 if dtype == torch.int8 else 32768
        shift = 1 if dtype == torch.int8 else -7
        nbytes = N * cpad * (esize * H * W + P * Q)
        nset = max(2, min(16, -(-600_000_000 // nbytes)))
        sets = [(torch.randint(-lim, lim, (N, H, W, cpad), dtype=dtype, device="cuda", generator=gen),
                 torch.empty(N, P, Q, cpad, dtype=torch.int8, device="cuda")) for _ in range(nset)]

        def launch(L, k):
            x, y = sets[k % nset]
            rc = getattr(L, entry)(x.data_ptr(), y.data_ptr(), N, H, W, C, cpad, kh, kw, sh, sw, ph, pw, 0, shift, 0, None)
            assert rc == 0, (name, rc)

        # equality of the two builds at the timed size
        got = {}
        for arm, L in libs.items():
            sets[0][1].fill_(77)
            launch(L, 0)
            torch.cuda.synchronize()
            got[arm] = sets[0][1].clone()
        equal = torch.equal(got["old"], got["new"]) and bool((got["new"][..., C:] == 0).all()) and int(got["new"].max()) > 0
        del got

        def timed(L, count):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(count):
                launch(L, k)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / count                   # microseconds per launch

        for L in libs.values():
            timed(L, 4 * nset)
        count = max(50, min(5000, int(30000.0 / max(timed(libs["old"], 4 * nset), 1.0))))
        t = {"old": [], "new": [], "old again": []}
        for _ in range(a.rounds):
            t["old"].append(timed(libs["old"], count))
            t["new"].append(timed(libs["new"], count))
            t["old again"].append(timed(libs["old"], count))
        say("%s: %.2f MB per launch, %d buffer sets, %d launches per round, outputs %s" % (name, nbytes / 1e6, nset, count, "equal" if equal else "DIFFER"))
        for arm in ("old", "new", "old again"):
            v = t[arm]
            med = statistics.median(v)
            say("    %-9s median %8.2f us  min %8.2f  max %8.2f  spread %6.2f  %.2f TB/s" % (arm, med, min(v), max(v), max(v) - min(v), nbytes / med / 1e6))
        old_med, new_med, spread = statistics.median(t["old"]), statistics.median(t["new"]), max(t["old"]) - min(t["old"])
        ok = new_med <= old_med + spread
        say("    new - old = %+.2f us (%+.2f %%), old arm's spread %.2f us: %s" % (new_med - old_med, 100 * (new_med - old_med) / old_med, spread, "within the rule" if ok else "MISSES the rule"))
        failed = failed or not ok or not equal
        del sets
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
