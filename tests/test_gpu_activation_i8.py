"""fq_act_lut_i8_nhwc on the GPU against its rule in numpy (activation_nets.act_lut_rule: table lookup plus zeroed padding), and
_native.build_act_table on the device against the CPU double of the same module.  Exact.    pytest -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import activation_doubles as ad
import activation_nets as an

pytestmark = pytest.mark.gpu


def _tables():
    rng = np.random.default_rng(7)
    sigmoid = ad.build_act_table(torch.nn.Sigmoid(), 4, 7).numpy()
    assert sigmoid[128] == 64                                # f(0) = 0.5: what a padding channel would read
    return {"identity": np.arange(-128, 128).astype(np.int8), "permutation": rng.permutation(256).astype(np.uint8).view(np.int8),
            "constant 77": np.full(256, 77, dtype=np.int8), "sigmoid (4, 7)": sigmoid}


@pytest.fixture(scope="module")
def tables(oracle):
    return _tables()


def _input(case, seed):
    """int8 [N, H, W, Cpad] holding every one of the 256 byte values where it has 256 bytes, padding channels included (the kernel
    must not let them through); smaller tensors are run several times with a different slice of the values each time."""
    n, h, w, _c, cpad = case
    size = n * h * w * cpad
    x = np.random.default_rng(seed).integers(-128, 128, size).astype(np.int8)
    vals = np.arange(-128, 128).astype(np.int8)
    if size >= 256:
        x[np.random.default_rng(seed + 1).permutation(size)[:256]] = vals
    else:
        x[:] = vals[(np.arange(size) + (seed - 11) * size) % 256]      # run `seed - 11` of ceil(256 / size): the next slice
    return x.reshape(n, h, w, cpad)


def _launch(nat, x, c, table):
    """The entry point itself, so that rows that are no multiple of 16 bytes can be passed (the binding takes pad16(c) only)."""
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(table).cuda()
    yd = torch.full_like(xd, 0x55)
    n, h, w, cpad = x.shape
    rc = nat.lib().fq_act_lut_i8_nhwc(xd.data_ptr(), yd.data_ptr(), td.data_ptr(), n, h, w, int(c), cpad, nat._stream(xd))
    assert rc == 0, rc
    return yd.cpu().numpy()


@pytest.mark.parametrize("case", an.KERNEL_CASES, ids=an.case_arg)
def test_the_kernel_is_the_table_lookup_with_zeroed_padding(case, tables):
    from common.quantity import _native as nat
    c, cpad = case[3], case[4]
    size = int(np.prod(case[:3])) * cpad
    seen = set()
    for rep in range(1 if size >= 256 else -(-256 // size)):
        x = _input(case, 11 + rep)
        seen |= set(int(v) for v in np.unique(x[..., :c]))
        for name, table in tables.items():
            got = _launch(nat, x, c, table)
            np.testing.assert_array_equal(got, an.act_lut_rule(x, c, table), err_msg="%s, table %s" % (case, name))
            assert not got[..., c:].any()
            if name == "constant 77":
                assert (got[..., :c] == 77).all()
    if size >= 256 and c == cpad:
        assert len(seen) == 256                              # every byte value went through the lookup
    if case == an.STRIDE_LOOP:
        assert size // 16 == an.BLOCK * an.MAX_BLOCKS + 1     # one chunk more than one pass of the capped grid


def test_the_inputs_hold_every_byte_value():
    for case in an.KERNEL_CASES:
        size = int(np.prod(case[:3])) * case[4]
        reps = 1 if size >= 256 else -(-256 // size)
        vals = set()
        for rep in range(reps):
            vals |= set(int(v) for v in _input(case, 11 + rep).ravel())
        assert len(vals) == 256, case


def test_the_binding_takes_the_projects_padding_and_refuses_any_other(tables):
    from common.quantity import _native as nat
    x = _input((2, 5, 5, 58, 64), 3)
    t = torch.from_numpy(tables["permutation"]).cuda()
    y = nat.act_lut_i8_nhwc(torch.from_numpy(x).cuda(), 58, t)
    np.testing.assert_array_equal(y.cpu().numpy(), an.act_lut_rule(x, 58, tables["permutation"]))
    out = torch.empty_like(y)
    assert nat.act_lut_i8_nhwc(torch.from_numpy(x).cuda(), 58, t, out=out) is out and torch.equal(out, y)
    with pytest.raises(nat.FqError):
        nat.act_lut_i8_nhwc(torch.from_numpy(x).cuda(), 40, t)            # 40 channels are stored as 48
    with pytest.raises(nat.FqError):
        nat.act_lut_i8_nhwc(torch.from_numpy(x), 58, t)                   # a host tensor
    # both forms of the lookup (csrc/fq_act_lut_i8.hip) give the same bytes
    fn = nat.lib().fq_debug_act_lut_i8_form
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    xd = torch.from_numpy(x).cuda()
    for form in (0, 1):
        yd = torch.full_like(xd, 0x55)
        assert fn(xd.data_ptr(), yd.data_ptr(), t.data_ptr(), 2, 5, 5, 58, 64, form, nat._stream(xd)) == 0
        assert torch.equal(yd, y), form


# Types whose device table differs from the CPU double's in some entry (a device tanh / exp that differs from the CPU's in the last
# bit, on a value that Quantity rounds the other way): for these the DEVICE chain is the truth and the table is held against the
# device's own elementwise DeQuantity -> module -> Quantity over 256 separate elements.  Recorded in DESIGN section 26.
DEVICE_IS_THE_TRUTH = ()


@pytest.mark.parametrize("name", list(an.ACTIVATIONS))
def test_the_device_table_is_the_cpu_doubles_entry_by_entry(name, oracle):
    from common.quantity import _native as nat
    m = an.ACTIVATIONS[name]().eval()
    md = an.ACTIVATIONS[name]().eval().cuda()
    for g, b in an.GRID_BIT_PAIRS:
        got = nat.build_act_table(md, g, b)
        assert got.is_cuda and got.dtype == torch.int8 and tuple(got.shape) == (256,)
        # the device's own chain, one element per launch shape [256, 1, 1, 1] (no [1, 1, 16, 16] broadcast to lean on)
        q = torch.arange(-128, 128, dtype=torch.float32, device="cuda").reshape(256, 1, 1, 1)
        with torch.no_grad():
            own = nat.quantity(md(nat.dequantity(q, g)).contiguous(), b).reshape(256).to(torch.int8)
        assert torch.equal(got, own), (name, g, b)
        want = ad.build_act_table(m, g, b).numpy()
        diff = np.flatnonzero(got.cpu().numpy() != want)
        print("%s (%d, %d): %d entries differ from the CPU double %s" % (name, g, b, diff.size, list(diff[:8] - 128)))
        if name not in DEVICE_IS_THE_TRUTH:
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg="%s (%d, %d)" % (name, g, b))
