"""scripts/recon_fuzz.py in its `shuffle` mode on the GPU: random nets of Slice markers and nn.ChannelShuffle modules
(tests/shuffle_nets.py: RandomShuffleNet) calibrated, rewritten and rebuilt as ReconModel; the resident plan with depthwise, concat,
flatten and shuffle on against fp32 module boundaries -- eagerly, captured as one HIP graph and as two half-batch graphs, at
another batch size and pickled: bit for bit.    pytest -m gpu"""
import importlib.util
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_resident_plans_of_random_shuffle_nets_keep_the_logits():
    rf = _script("recon_fuzz")
    found = []
    bad, seen = rf.run(10, 23, log=found.append, shuffle=True)
    assert bad == 0, found
    assert seen["shuffle_modules"] > 20 and seen["resident_shuffles"] + seen["resident_slices"] > 10, seen
    assert seen["resident_shuffles"] + seen["resident_slices"] + seen["shuffles_left"] == seen["shuffle_modules"], seen
