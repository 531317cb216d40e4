"""Twelve random integer-simulation nets (requant_nets.RandomRequantNet) on the MI355X under
resident.enable(concat=True, requant=True): run eagerly, as one HIP graph and pickled, exact outputs.   pytest -m gpu"""
import io
import pickle

import pytest
import torch

import requant_nets as rn

pytestmark = pytest.mark.gpu

SEEDS = list(range(100, 112))


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_requant_eager_graphed_and_pickled(seed):
    from common.quantity import resident
    net = rn.RandomRequantNet(seed).cuda().eval()
    x, x2 = net.example(1).cuda(), net.example(2).cuda() * 1.5
    with torch.no_grad():
        plain, plain2 = tuple(t.clone() for t in net(x)), tuple(t.clone() for t in net(x2))
    want = sum(1 for _n, kind in net.cats if kind in rn.CAUSES)
    off = resident.enable(net, x, concat=True)
    assert "requant_concats" not in off
    with torch.no_grad():
        assert _same(net(x), plain)
    on = resident.enable(net, x, concat=True, requant=True)                     # verify=True
    plans = resident.describe(net)
    assert on["requant_concats"] == want, (on, net.cats, plans.requant_left)
    assert set(plans.requant_left) == set(n for n, kind in net.cats if kind == "declined")
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
