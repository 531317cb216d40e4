"""bench.py's plain run (no --full) on hardware: exactly one JSON line with the headline keys and none of what --full adds, and
--dump-outputs writing what the timed calibration computed, each array tied to evidence of its own: absmax and hist are what
the line's statistics_sha256 digests, bits rebuild the feat.table the line's feat_table_sha256 digests, every threshold is the
CPU oracle's KL threshold bin of its dumped histogram at the interval of its dumped maximum; and a second process with the
same arguments dumps the same arrays.   pytest -m gpu"""
import contextlib
import hashlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--images", "64", "--steps", "2", "--warmup", "1"]
DUMPED = ("bits", "absmax", "hist", "threshold")


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().split("\n") if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {n: np.load(os.path.join(str(out_dir), n + ".npy")) for n in DUMPED}


def _r50_graph():
    """The bench's ResNet-50 as the calibration sees it: rows, names, inputs and merge groups (discovered on the CPU: they do
    not depend on the device)."""
    import torch
    import bench
    from tools import Quantity
    from workdir_util import product_workdir
    with contextlib.redirect_stdout(io.StringIO()), product_workdir(input_shape="1,3,224,224", device="cpu"):
        q = Quantity(bench.build_model("r50", 224, torch.device("cpu")))
        groups = q.get_merge_groups(q.net_info)
    return q, groups


def _feat_table(q, bits):
    """feat.table as Quantity.activation_quantize writes it, from one bit per row."""
    names = ["image"] + list(q.net_info)
    assert len(names) == len(bits)
    b = {n: str(int(v)) for n, v in zip(names, bits)}
    lines = ["image " + b["image"], " ".join([q.cared_op_layer_names[0], b[names[1]], b["image"]])]
    for i, n in enumerate(names[2:], 1):
        lines.append(" ".join([q.cared_op_layer_names[i], b[n]] + [b[s] for s in q.net_info[n]["inputs"]]))
    return "".join(line + "\n" for line in lines)


@pytest.mark.timeout(1200)
def test_plain_bench_times_the_steps_and_dumps_what_they_computed(tmp_path, oracle):
    d, a = _plain_run(tmp_path / "a")
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["value"] > 0
    assert d["steps"] == 2 and d["warmup"] == 1 and d["config"]["batch"] == 32 and d["ms_per_step"] > 0
    assert d["own_conv_launches"] == d["expected_own_conv_launches"] == 53 * 2 and "error" not in d
    for key in ("value_cold", "split_bf16", "roofline_bias_add_absmax", "roofline_fakequant", "int8_sim_images_per_s",
                "cpu_baseline", "file_input", "per_channel_calibration"):
        assert key not in d, key                           # measured with --full only
    rows = a["absmax"].shape[0]
    assert a["absmax"].dtype == np.float32 and a["hist"].shape == (rows, 2048) and a["hist"].dtype == np.float64
    assert a["bits"].shape == a["threshold"].shape == (rows,) and a["bits"].dtype == a["threshold"].dtype == np.float64
    assert np.all(a["absmax"] > 0) and np.all(a["threshold"] > 0)
    digest = hashlib.sha256(a["absmax"].tobytes() + a["hist"].astype(np.int64).tobytes()).hexdigest()
    assert digest == d["statistics_sha256"]
    q, groups = _r50_graph()
    assert hashlib.sha256(_feat_table(q, a["bits"]).encode()).hexdigest() == d["feat_table_sha256"]
    # every row's interval from its maximum; a merge group that does not feed an Eltwise (a projection block's conv3 and
    # shortcut) shares its widest interval and is searched on the sum of its members' histograms
    row = {n: i for i, n in enumerate(["image"] + list(q.net_info))}
    iv = np.array([oracle.interval(m) for m in a["absmax"]], dtype=np.float64)
    hist = a["hist"].astype(np.int64)
    widened = 0
    for g in groups:
        if not q._group_has_eltwise(g):
            idx = [row[n] for n in g]
            iv[idx] = iv[idx].max()
            hist[idx] = hist[idx].sum(axis=0)
            widened += 1
    assert widened == 4                                    # ResNet-50: one projection block per stage
    t = np.array([oracle.kl_threshold(oracle.normalize(h), use_fq_log=True) for h in hist])
    assert np.array_equal(np.rint(a["threshold"] / iv - 0.5), t)
    np.testing.assert_allclose(a["threshold"], (t + 0.5) * iv, rtol=1e-6, atol=0)
    # same arguments, same inputs: a second process computes the same arrays
    d2, b = _plain_run(tmp_path / "b")
    for n in DUMPED:
        assert np.array_equal(a[n], b[n]), n
    assert (d2["statistics_sha256"], d2["feat_table_sha256"]) == (d["statistics_sha256"], d["feat_table_sha256"])
