"""Twelve random U-Net-shaped integer-simulation nets (bilinear_nets.RandomBilinearNet) on the MI355X under
resident.enable(concat=True, bilinear=True): run eagerly, as one HIP graph and pickled, exact outputs.   pytest -m gpu"""
import io
import pickle

import pytest
import torch

import bilinear_nets as bn

pytestmark = pytest.mark.gpu

SEEDS = list(range(100, 112))


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_bilinear_eager_graphed_and_pickled(seed):
    from common.quantity import resident
    net = bn.RandomBilinearNet(seed).cuda().eval()
    x, x2 = net.example(1).cuda(), net.example(2).cuda() * 1.5
    with torch.no_grad():
        plain, plain2 = tuple(t.clone() for t in net(x)), tuple(t.clone() for t in net(x2))
    want = sum(1 for _n, ok in net.ups if ok)
    assert len(net.ups) >= 1
    off = resident.enable(net, x, concat=True)
    assert "resident_bilinears" not in off
    with torch.no_grad():
        assert _same(net(x), plain)
    on = resident.enable(net, x, concat=True, bilinear=True)                    # verify=True
    plans = resident.describe(net)
    assert on["resident_bilinears"] == want, (on, net.ups, plans.bilinear_left)
    assert set(plans.bilinear_left) == set(n for n, ok in net.ups if not ok)
    with torch.no_grad():
        assert _same(net(x), plain) and _same(net(x2), plain2)
        assert _same(net(x[:1]), tuple(p[:1] for p in plain))
        assert _same(net(torch.flip(x, dims=[0])), tuple(torch.flip(p, dims=[0]) for p in plain))
        buf = io.BytesIO()
        pickle.dump(net, buf)
        again = pickle.loads(buf.getvalue())
        assert _same(again(x2), plain2) and resident.describe(again).keys() == plans.keys()
    graphed = resident.GraphedForward(net, x)
    assert _same(graphed(x), plain)
    assert _same(graphed(x2), plain2)
    assert _same(graphed(x), plain)
