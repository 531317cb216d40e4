"""The family of tests/test_mixed_plan_cpu.py on the HIP kernels: the same random mixed graphs, the same
CPU-calibrated tables, so the plans are the ones the CPU suite checked on the doubles.  Per model: the logits with fp32 module
boundaries from the oracle-backed doubles on the host and from the library on the GPU, and with all eight switches on the planned
logits -- eager on the example batch, on another batch and at another batch size, as one HIP graph, as two graphs on two streams,
pickled and loaded -- all equal bit for bit; and the GPU plan's summary is the one the doubles gave, which carries the coverage
conditions of the CPU test over.  No kernel has a test of its own here: the launches take argument combinations that no per-kernel
test uses (a table over the padded output of a slice of a grouped layer, an eight-source Concat with clipped and unclipped leaves).

The two unplanned chains differ in the library's ops alone: the oracle-backed doubles on the host, the HIP kernels on the GPU.  The ops
that stay torch's in both -- the table activations and nn.AvgPool2d on fp32 tensors -- run on the GPU's torch kernels in the host
chain too (torch_ops_on_the_gpu).  torch's own CPU and GPU kernels of these ops are one ulp apart: measured on this family, nn.Tanh
on 3371 of 32768 elements, nn.Hardsigmoid on 2472 of 8192, nn.Hardswish on 640 of 6144, nn.Sigmoid on 404 of 5120, all by at most
2^-23 relative; behind a fp32 average pool that moved the logits of model 27 (2.5625 against 2.5000).  Neither is the library's."""
import contextlib
import io
import json
import time

import pytest
import torch
from torch import nn

import all_doubles
import mixed_nets as mn

CHUNK = 2                                                     # models per test: each test stays within a few seconds
FAMILY = mn.family()
CHUNKS = [FAMILY[k:k + CHUNK] for k in range(0, len(FAMILY), CHUNK)]


@contextlib.contextmanager
def torch_ops_on_the_gpu(net):
    """The modules of the host model `net` that are torch's own fp32 ops on values off the integer grid -- table activations, average
    pools -- compute on the GPU for the duration: the same torch kernels as in the model that runs on the library."""
    from common.quantity import resident

    def on_gpu(m):
        def forward(x):
            y = type(m).forward(m, x.cuda()).cpu()
            return x.copy_(y) if getattr(m, "inplace", False) else y
        return forward
    mods = [m for m in net.modules() if resident._is_table_activation(m) or isinstance(m, nn.AvgPool2d)]
    for m in mods:
        m.__dict__["forward"] = on_gpu(m)
    try:
        yield
    finally:
        for m in mods:
            del m.__dict__["forward"]


def check_on_gpu(index, seed):
    """-> (summary of the GPU plan, {what was left: how many}) of model `index`, after every comparison."""
    from common.quantity import resident
    info, (host, dev) = mn.calibrated(index, seed, [all_doubles.installed, contextlib.nullcontext])
    x, x2 = mn.inputs(host, index, seed)
    with all_doubles.installed(), torch.no_grad():
        with torch_ops_on_the_gpu(host):
            want = [host(x), host(x2), host(x[:3])]
        host_summary = resident.enable(host, x, **mn.ALL_SWITCHES)
    tag = "model %d" % index
    dev = dev.cuda()
    xg, xg2 = x.cuda(), x2.cuda()
    with torch.no_grad():
        plain = [dev(xg), dev(xg2), dev(xg[:3])]
        for got, ref in zip(plain, want):
            assert torch.equal(got.cpu(), ref), tag + ": the library's logits are not the doubles'"
        summary = resident.enable(dev, xg, **mn.ALL_SWITCHES)
        assert summary == host_summary, (tag, summary, host_summary)
        assert torch.equal(dev(xg), plain[0]), tag
        assert torch.equal(dev(xg2), plain[1]), tag + " (another batch)"
        assert torch.equal(dev(xg[:3]), plain[2]), tag + " (another batch size)"
        graphed = resident.capture(dev, xg)
        assert torch.equal(graphed(xg), plain[0]) and torch.equal(graphed(xg2), plain[1]), tag + " (one graph)"
        dual = resident.capture(dev, xg, streams=2)
        assert torch.equal(dual(xg), plain[0]) and torch.equal(dual(xg2), plain[1]), tag + " (two graphs on two streams)"
        buf = io.BytesIO()
        torch.save(dev, buf)
        buf.seek(0)
        again = torch.load(buf, weights_only=False)
        assert torch.equal(again(xg2), plain[1]), tag + " (pickled)"
        plans = resident.describe(dev)
        left = {"activations_left": len(plans.activations_left), "shuffle_left": len(plans.shuffle_left),
                "relu6_left": len(plans.relu6_left)}
        resident.disable(dev)
        assert torch.equal(dev(xg), plain[0]), tag + " (disabled)"
    return summary, left


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
def test_mixed_graphs_with_every_switch_on_keep_their_logits_on_the_gpu(chunk, oracle):
    start = time.perf_counter()
    total = {}
    for index, seed in CHUNKS[chunk]:
        summary, left = check_on_gpu(index, seed)
        for k, v in list(summary.items()) + list(left.items()):
            total[k] = total.get(k, 0) + v
    torch.cuda.synchronize()
    # (a record for profiles/r18_mixed_fuzz.txt; nothing asserts on time)
    print("mixed_fuzz chunk %d %s" % (chunk, json.dumps({"models": [i for i, _s in CHUNKS[chunk]],
                                                          "seconds": round(time.perf_counter() - start, 2), "plan": total})))


@pytest.mark.gpu
def test_g22_logits_on_the_gpu_plain_and_with_every_switch_on(oracle, golden_dir):
    """Golden G22: the reference's own ReconModel logits of the mixed graphs it accepts, from the integer-simulation model on the HIP
    kernels, built from the tables of the oracle-backed CPU calibration (which the CPU test pins to the reference's byte for byte):
    with fp32 module boundaries and with all eight switches on, bit for bit."""
    import os
    import numpy as np
    from common.quantity import resident
    with open(os.path.join(golden_dir, "g22_mixed_graphs.json")) as fh:
        ref = json.load(fh)
    arrays = np.load(os.path.join(golden_dir, "g22_mixed_graphs.npz"))
    checked = 0
    for tag in sorted(ref, key=int):
        if "reference_error" in ref[tag]:
            continue
        index, seed = int(tag), mn.FAMILY_SEED
        _info, (net,) = mn.calibrated(index, seed, [contextlib.nullcontext])
        x, _x2 = mn.inputs(net, index, seed)
        net, x = net.cuda(), x.cuda()
        want = arrays["logits_%s" % tag]
        with torch.no_grad():
            np.testing.assert_array_equal(net(x).cpu().numpy(), want, err_msg=tag)
            resident.enable(net, x, **mn.ALL_SWITCHES)
            np.testing.assert_array_equal(net(x).cpu().numpy(), want, err_msg=tag + " (every switch on)")
        checked += 1
    assert checked >= 6
