"""Twenty random ResNet-D-shaped integer-simulation nets (sum_pool_nets.RandomResNetD) on the MI355X under
resident.enable(avgpool=True, sums=True): run eagerly and as one HIP graph, exact logits.   pytest -m gpu"""
import pytest
import torch

import sum_pool_nets as sn

pytestmark = pytest.mark.gpu

SEEDS = list(range(100, 120))


def _tuple(t):
    return t if isinstance(t, tuple) else (t,)


def _same(a, b):
    a, b = _tuple(a), _tuple(b)
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_resnet_d_eager_and_graphed(seed):
    from common.quantity import resident
    net = sn.RandomResNetD(seed).cuda().eval()
    x, x2 = net.example(1).cuda(), net.example(2).cuda() * 1.5
    with torch.no_grad():
        plain, plain2 = tuple(t.clone() for t in _tuple(net(x))), tuple(t.clone() for t in _tuple(net(x2)))
    want = sum(1 for _n, ok in net.pools if ok)
    assert len(net.pools) >= 1
    off = resident.enable(net, x, avgpool=True)
    on = resident.enable(net, x, avgpool=True, sums=True)                       # verify=True
    plans = resident.describe(net)
    assert on["resident_sum_avgpools"] == want and on["fp32_outputs"] == off["fp32_outputs"] - want, (off, on, plans.avgpool_left)
    assert set(plans.avgpool_left) == set(n for n, ok in net.pools if not ok)
    with torch.no_grad():
        assert _same(net(x), plain) and _same(net(x2), plain2)
        assert _same(net(x[:1]), tuple(p[:1] for p in plain))
        assert _same(net(torch.flip(x, dims=[0])), tuple(torch.flip(p, dims=[0]) for p in plain))
    graphed = resident.GraphedForward(net, x)
    assert _same(graphed(x), plain)
    assert _same(graphed(x2), plain2)
    assert _same(graphed(x), plain)
