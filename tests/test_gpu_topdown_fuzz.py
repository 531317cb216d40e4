"""Twenty random FPN-shaped integer-simulation nets (topdown_nets.RandomTopDown) on the MI355X under
resident.enable(concat=True, topdown=True): run eagerly and as one HIP graph, exact outputs.   pytest -m gpu"""
import pytest
import torch

import topdown_nets as tn

pytestmark = pytest.mark.gpu

SEEDS = list(range(100, 120))


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_topdown_eager_and_graphed(seed):
    from common.quantity import resident
    net = tn.RandomTopDown(seed).cuda().eval()
    x, x2 = net.example(1).cuda(), net.example(2).cuda() * 1.5
    with torch.no_grad():
        plain, plain2 = tuple(t.clone() for t in net(x)), tuple(t.clone() for t in net(x2))
    want = sum(1 for _n, ok, _s in net.ups if ok)
    assert len(net.ups) >= 1
    resident.enable(net, x, concat=True)
    with torch.no_grad():
        assert _same(net(x), plain)
    on = resident.enable(net, x, concat=True, topdown=True)                     # verify=True
    plans = resident.describe(net)
    assert on["topdown_adds"] == want, (on, net.ups, plans.topdown_left)
    assert on["topdown_sum_sources"] == sum(1 for _n, ok, s in net.ups if ok and s)
    assert set(plans.topdown_left) == set(n for n, ok, _s in net.ups if not ok)
    with torch.no_grad():
        assert _same(net(x), plain) and _same(net(x2), plain2)
        assert _same(net(x[:1]), tuple(p[:1] for p in plain))
        assert _same(net(torch.flip(x, dims=[0])), tuple(torch.flip(p, dims=[0]) for p in plain))
    graphed = resident.GraphedForward(net, x)
    assert _same(graphed(x), plain)
    assert _same(graphed(x2), plain2)
    assert _same(graphed(x), plain)
