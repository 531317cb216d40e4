"""Small residual models for the tests of the fused calibration forward's host bookkeeping (tools/_fused_forward.py,
tools/_hook_state.py): the two-block net of tests/test_gpu_conv_add_fusion.py, and a three-block net whose forward writes to one
of its own tensors in place at a chosen SITE -- always, or only from the second calibration batch on, when both probe forwards
and the first batch have already shown the calibration a clean model (tests/test_gpu_calib_inplace.py)."""
import contextlib
import os

import cases
from workdir_util import product_workdir


def _block_net(variant="plain", hw=64):
    """stem -> 2 x [1x1 -> ReLU -> 3x3 -> ReLU -> 1x1 (128 channels)] + shortcut -> Eltwise -> ReLU -> pool -> fc.
    variant "peek": block 1's convolution output is ALSO read by something else before its Eltwise;
    variant "inplace_relu": the ReLU behind the Eltwise works in place."""
    from torch import nn
    from common.quantity import Eltwise, View

    class Block(nn.Module):
        def __init__(self, cin, mid, cout, stride, peek):
            super().__init__()
            self.c1, self.r1 = nn.Conv2d(cin, mid, 1), nn.ReLU()
            self.c2, self.r2 = nn.Conv2d(mid, mid, 3, stride=stride, padding=1), nn.ReLU()
            self.c3 = nn.Conv2d(mid, cout, 1)
            self.down = nn.Conv2d(cin, cout, 1, stride=stride) if (stride != 1 or cin != cout) else None
            self.add = Eltwise()
            self.r3 = nn.ReLU(variant == "inplace_relu")
            self.peek = (nn.ReLU(), Eltwise()) if peek else None
            if peek:
                self.peek_relu, self.peek_add = self.peek

        def forward(self, x):
            y = self.c3(self.r2(self.c2(self.r1(self.c1(x)))))
            side = self.peek_relu(y) if self.peek else None                    # a second reader of the convolution's output
            z = self.r3(self.add(y, x if self.down is None else self.down(x)))
            return z if side is None else self.peek_add(z, side)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem, self.relu0 = nn.Conv2d(3, 32, 3, padding=1), nn.ReLU()
            self.b1 = Block(32, 16, 128, 2, peek=False)
            self.b2 = Block(128, 32, 128, 1, peek=variant == "peek")
            self.pool, self.view, self.fc = nn.AvgPool2d(hw // 2), View(), nn.Linear(128, 10)

        def forward(self, x):
            return self.fc(self.view(self.pool(self.b2(self.b1(self.relu0(self.stem(x)))))))
    return Net()


def _calibrate(model, fuse, cache_gb=None, plan="", batches=5, monkeypatch=None, hw=64, skip=None, pair=None, chain=None):
    from tools import Quantity
    if monkeypatch is not None and cache_gb is not None:
        monkeypatch.setenv("FQ_ACT_CACHE_GB", cache_gb)
        monkeypatch.setenv("FQ_CACHE_PLAN", plan)
    with product_workdir(input_shape="1,3,%d,%d" % (hw, hw), device="gpu", max_cali_img_num=batches - 1) as tmp:
        q = Quantity(model)
        q.fuse_conv_add = fuse
        q.skip_unread_outputs = fuse if skip is None else skip
        if pair is not None:
            q.pair_hist = pair
        if chain is not None:
            q.pair_chain = chain
        bits = q.activation_quantize(cases.calib_batches(batches, (8, 3, hw, hw), seed=91))
        table = open(os.path.join(tmp, "test", "workdir", "feat.table")).read()
        return dict(bits), table, dict(q._collector.max_vals), q._collector.hist_device.clone(), dict(q.timings)


# ---- a chain of three sums, written to in place --------------------------------------------------------------------------------
# site -> which tensor the model writes to, and where (every write is exact in fp32: * 0.5, + 1.0)
SITES = ("none",
         "relu_before_add",           # b1's ReLU output = b2's input and shortcut, right after b1.r3, by a tensor method
         "relu_before_add_module",    # the same, by an in-place nn.Module of a type configs.yml does not list, between the blocks
         "relu_view_before_add",      # the same, through a view (z[:]); b2 is given the base
         "relu_after_next_add",       # b1's ReLU output after b2's add, while b3 is chained on b2
         "conv3_after_add",           # b2.c3's output (hooked, deferred to the add) after b2.add
         "sum_after_relu",            # b2.add's output (hooked; not written at all when its pair is left to pass 2) after b2.r3 read it
         "c1_after_relu",             # b2.c1's output (hooked, a convolution only its ReLU reads) after b2.r1 read it
         "projection_after_add")      # b1.down's output (hooked, kept; the shortcut of a pair that is no chain link) after b1.add

BATCH_SHAPE = (4, 3, 32, 32)          # 16 x 16 planes behind b1: the one-kernel tail with its sum left to pass 2
N_BATCHES = 3


def chain_batches():
    return cases.calib_batches(N_BATCHES, BATCH_SHAPE, seed=91)


def _tag(images):
    """What tells one batch from another (and from the probes' random input) inside the model: its first pixel."""
    return float(images.flatten()[0])


def chain_net(site="none", when="always", batches=None):
    """stem -> b1 (projection block, stride 2) -> b2 -> b3 (identity blocks) -> pool -> fc: three residual sums, S_2's shortcut
    relu(S_1) and S_3's relu(S_2), so that a wrong relu(S_1) in pass 2 shows in the histograms of S_2 AND S_3.
    The forward writes in place at `site`:
      when = "always"  in every forward -- the trace, both probe forwards and every batch: the calibration can know;
      when = "later"   only in the forwards of batches 1.. of `batches`: the trace, the probes and batch 0 see a clean model.
    ("later" is a function of the forward's INPUT, not of a call counter as in test_an_input_written_in_place_before_the_eltwise_is_
    refused: the arms of a comparison run different numbers of probe forwards, and an arm without a cache runs every batch again in
    pass 2 -- the same batch must meet the same model in every arm and in both passes.)"""
    from torch import nn
    from common.quantity import Eltwise, View
    assert site in SITES and when in ("always", "later")
    late = frozenset(_tag(b[0]) for b in (batches or [])[1:])
    assert when == "always" or late
    live = {"on": False}

    class HalveInPlace(nn.Module):                          # (not a type the graph discovery or the hooks know)
        def forward(self, x):
            return x.mul_(0.5)

    class Block(nn.Module):
        def __init__(self, cin, mid, cout, stride, sites):
            super().__init__()
            self.c1, self.r1 = nn.Conv2d(cin, mid, 1), nn.ReLU()
            self.c2, self.r2 = nn.Conv2d(mid, mid, 3, stride=stride, padding=1), nn.ReLU()
            self.c3 = nn.Conv2d(mid, cout, 1)
            self.down = nn.Conv2d(cin, cout, 1, stride=stride) if (stride != 1 or cin != cout) else None
            self.add, self.r3 = Eltwise(), nn.ReLU()
            self.sites = sites

        def forward(self, x):
            writes = self.sites if live["on"] else ()
            t = self.c1(x)
            a = self.r1(t)
            if "c1_after_relu" in writes:
                t.mul_(0.5)
            y = self.c3(self.r2(self.c2(a)))
            shortcut = x if self.down is None else self.down(x)
            s = self.add(y, shortcut)
            if "conv3_after_add" in writes:
                y.mul_(0.5)
            if "projection_after_add" in writes:
                shortcut.add_(1.0)
            z = self.r3(s)
            if "sum_after_relu" in writes:
                s.mul_(0.5)
            return z

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem, self.relu0 = nn.Conv2d(3, 32, 3, padding=1), nn.ReLU()
            self.b1 = Block(32, 16, 128, 2, (site,) if site == "projection_after_add" else ())
            self.b2 = Block(128, 32, 128, 1, (site,) if site in ("conv3_after_add", "sum_after_relu", "c1_after_relu") else ())
            self.b3 = Block(128, 32, 128, 1, ())
            self.meddle = HalveInPlace()
            self.pool, self.view, self.fc = nn.AvgPool2d(BATCH_SHAPE[2] // 2), View(), nn.Linear(128, 10)
            self.tag = None                                 # of the running forward's input

        def forward(self, x):
            self.tag = _tag(x)
            live["on"] = on = when == "always" or self.tag in late
            z1 = self.b1(self.relu0(self.stem(x)))
            if on and site == "relu_before_add":
                z1.mul_(0.5)
            elif on and site == "relu_before_add_module":
                z1 = self.meddle(z1)
            elif on and site == "relu_view_before_add":
                z1[:].mul_(0.5)
            z2 = self.b2(z1)
            if on and site == "relu_after_next_add":
                z1.mul_(0.5)
            return self.fc(self.view(self.pool(self.b3(z2))))
    return Net()


# name -> (FQ_ACT_CACHE_GB, FQ_CACHE_PLAN, switches).  "reference": the product's plainest path on the same convolution kernels --
# no residual tail in one kernel, every output written, every sum written, one statistics launch per tensor from inside its hook,
# no cache: each tensor is counted when its module returns it, and pass 2 runs every forward again.
ARMS = {
    "reference": ("0", "", dict(fuse_conv_add=False, skip_unread_outputs=False, pair_hist=False, stats_group_bytes=0)),
    "A": ("1", "A", dict(fuse_conv_add=True, skip_unread_outputs=True, pair_hist=True, pair_chain=True)),
    "B": ("0.02", "B", dict(fuse_conv_add=True, skip_unread_outputs=True, pair_hist=True, pair_chain=True)),
    "A_flat": ("1", "A", dict(fuse_conv_add=True, skip_unread_outputs=True, pair_hist=True, pair_chain=False)),
}


@contextlib.contextmanager
def _environ(**values):
    old = dict((k, os.environ.get(k)) for k in values)
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def calibrate_chain(site, when, arm, tape=None, **switches):
    """One calibration of chain_net(site, when) (same weights and batches for every site and arm) under ARMS[arm] (+ `switches`).
    Returns a dict: bits, table (feat.table's text), max (every abs-max), hist (int64 [rows, 2048], on the host), timings, interval
    and row (per hooked tensor's key) and key (module name -> the key of its output).
    tape = {}: filled with (batch index, key) -> a clone of that hooked module's output, taken by a forward hook that runs AFTER
    the calibration's own hook of the same call (whose kernel is what fills the tensor), the first time each batch passes."""
    from tools import Quantity
    batches = chain_batches()
    model = cases.seed_model(chain_net(site, when, batches), base_seed=8).eval().cuda()
    cache_gb, plan, arm_switches = ARMS[arm]
    with _environ(FQ_ACT_CACHE_GB=cache_gb, FQ_CACHE_PLAN=plan), \
            product_workdir(input_shape="1,3,%d,%d" % BATCH_SHAPE[2:], device="gpu", max_cali_img_num=N_BATCHES - 1) as tmp:
        q = Quantity(model)
        for name, value in dict(arm_switches, **switches).items():
            assert hasattr(q, name), name
            setattr(q, name, value)
        key_of, handles = {}, []
        index_of = dict((_tag(b[0]), i) for i, b in enumerate(batches))
        if tape is not None:
            count = {"n": 0}
            module_name = dict((m, n) for n, m in model.named_modules())

            def on_forward(module, inputs, output):
                if module is model.stem:
                    count["n"] = 0
                count["n"] += 1
                key = "%s_%i" % (type(module).__name__, count["n"])
                if key in q.net_info:
                    key_of[module_name[module]] = key
                    if model.tag in index_of:
                        tape.setdefault((index_of[model.tag], key), output.detach().clone())
            real = q.regist_hook_outfeature

            def regist(m):
                out = real(m)
                for mod in m.modules():
                    if type(mod).__name__ in q._all_op_type:
                        handles.append(mod.register_forward_hook(on_forward))
                return out
            q.regist_hook_outfeature = regist
        try:
            bits = q.activation_quantize(batches)
        finally:
            for h in handles:
                h.remove()
        coll = q._collector
        names = ["image"] + list(q.net_info.keys())
        return {"bits": dict(bits), "table": open(os.path.join(tmp, "test", "workdir", "feat.table")).read(),
                "max": dict(coll.max_vals), "hist": coll.hist_device.cpu(), "timings": dict(q.timings),
                "interval": dict(coll._distribution_intervals), "row": dict((n, coll.row_of(n)) for n in names), "key": key_of}
