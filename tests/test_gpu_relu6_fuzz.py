"""The two GPU fuzzers in their `relu6` mode (about half of the nn.ReLU modules of every random topology become nn.ReLU6), everything
on against everything off: scripts/model_fuzz.py -- the calibration with fuse_relu6, own_depthwise and own_grouped against the
library path -- and scripts/recon_fuzz.py -- the resident plan with every opt-in argument against fp32 module boundaries, eagerly,
captured as a graph, at another batch size and pickled: bit for bit.    pytest -m gpu"""
import importlib.util
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    if name == "model_fuzz":
        sys.modules.setdefault("model_fuzz", mod)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("odd", [False, True], ids=["plain", "odd"])
def test_calibrations_of_random_topologies_with_relu6_give_the_unfused_tables(odd):
    mf = _script("model_fuzz")
    found = []
    bad, seen = mf.run(16, 61, log=found.append, odd=odd, relu6=True)
    assert bad == 0, [m for m in found if not m.startswith("  (")]
    assert seen["relu6_modules"] > 30 and seen["fused_relus"] > 0 and seen["own_conv1x1_launches"] > 0, seen


@pytest.mark.parametrize("odd", [False, True], ids=["plain", "odd"])
def test_resident_plans_of_random_topologies_with_relu6_keep_the_logits(odd):
    rf = _script("recon_fuzz")
    found = []
    bad, seen = rf.run(16, 62, log=found.append, odd=odd, relu6=True)
    assert bad == 0, found
    assert seen["relu6_modules"] > 30 and seen["fused_relu6s"] > 10 and seen["fused_relus"] > 10, seen
