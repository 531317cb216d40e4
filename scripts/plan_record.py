"""Record what resident.enable() plans in every CPU plan test, for a before / after comparison of a planner refactor.

    python scripts/plan_record.py OUT.json [pytest arguments; default: every tests/test_*_plan_cpu.py]

Runs the files in this process through pytest.main with resident.enable wrapped; pytest's configuration is untouched.  Per test id
and call index the record holds the summary as an ordered list of items (or the exception's type and text), repr of every Plan of
describe(), every report attribute of describe(), and the class of every instance-level forward on the model.  Two checkouts that
plan alike write identical files (compare them with cmp or diff)."""
import functools
import glob
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-quantity_amd", "quantity"))


class Recorder(object):
    def __init__(self, resident):
        self.resident, self.enable, self.test, self.record = resident, resident.enable, None, {}
        self.reports = sorted(k for k, v in vars(resident._Description).items() if not k.startswith("_") and not callable(v))

    def pytest_runtest_logstart(self, nodeid, location):
        self.test = nodeid

    def __call__(self, model, *args, **kwargs):
        calls = self.record.setdefault(self.test, [])
        entry = {}
        calls.append(entry)
        try:
            summary = self.enable(model, *args, **kwargs)
        except Exception as e:
            entry["raised"] = [type(e).__name__, str(e)]
            raise
        d = self.resident.describe(model)
        entry["summary"] = [[k, v] for k, v in summary.items()]
        entry["plans"] = [[name, repr(plan)] for name, plan in d.items()]
        entry["reports"] = dict((k, repr(getattr(d, k))) for k in self.reports)
        entry["forwards"] = [[name, type(m.__dict__["forward"]).__name__] for name, m in model.named_modules()
                             if isinstance(m.__dict__.get("forward"), self.resident._InstanceForward)]
        return summary


def main(argv):
    out = argv[0]
    files = argv[1:] or sorted(glob.glob(os.path.join(ROOT, "tests", "test_*_plan_cpu.py")))
    from common.quantity import resident
    recorder = Recorder(resident)
    resident.enable = functools.wraps(resident.enable)(lambda *args, **kwargs: recorder(*args, **kwargs))     # (keeps the signature)
    try:
        status = pytest.main(["-q", "-p", "no:cacheprovider"] + files, plugins=[recorder])
    finally:
        resident.enable = recorder.enable
    with open(out, "w") as f:
        json.dump(recorder.record, f, indent=1, sort_keys=True)
    print("%d enable() calls in %d tests -> %s" % (sum(len(c) for c in recorder.record.values()), len(recorder.record), out))
    return int(status)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
