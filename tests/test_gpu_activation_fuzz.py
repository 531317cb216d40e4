"""scripts/recon_fuzz.py in its `act` mode on the GPU: random nets of listed activations behind random convolutions, with a
max-pool, a Slice or a Concat behind some of them (tests/activation_nets.py: RandomActNet), calibrated, rewritten and rebuilt as
ReconModel; the resident plan with concat, shuffle and activations on against fp32 module boundaries -- eagerly, captured as one
HIP graph and as two half-batch graphs, at another batch size and pickled: bit for bit.    pytest -m gpu"""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS, SEED = 40, 31


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_resident_plans_of_random_activation_nets_keep_the_logits():
    rf = _script("recon_fuzz")
    found = []
    bad, seen = rf.run(MODELS, SEED, log=found.append, act=True)
    assert bad == 0, found
    # at least half of the models planned one or more activations: the test cannot pass by planning nothing
    assert seen["models_with_a_table"] >= MODELS // 2, seen
    assert seen["resident_activations"] + seen["acts_left"] == seen["act_modules"], seen
