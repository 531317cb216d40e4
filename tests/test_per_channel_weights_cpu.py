"""Per-channel weight bits, host side (no GPU): the weight_channel.table grammar and its reader, the per-channel MAX_SHIFT cap,
the per-channel rescale of the JSON integers, Quantity.weight_quantize_per_channel with the statistics engine replaced by
oracle-backed doubles (tests/engine_doubles.py), and Reconstruction.get_quantity_information_per_channel."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases
from engine_doubles import OracleCollector, OracleQuantizer
from per_channel_chain import dilate_dense, numpy_channel_bits
from workdir_util import product_workdir


def _write(path, text):
    with open(path, "w") as fh:
        fh.write(text)


def test_channel_table_reader_grammar(tmp_path):
    from common.quantity import BitReader
    p = str(tmp_path / "weight_channel.table")
    _write(p, "conv1.weight 5 6 7\nconv1.bias 3\nfc.weight 9\nfc.bias -2\n\n")
    wb, bb = BitReader(weight_table=p).get_weight_channel_info()
    assert list(wb.items()) == [("conv1", [5, 6, 7]), ("fc", [9])]
    assert list(bb.items()) == [("conv1", 3), ("fc", -2)]
    _write(p, "conv1.weight 5\nconv1.bias 3 4\n")
    with pytest.raises(ValueError):
        BitReader(weight_table=p).get_weight_channel_info()
    _write(p, "conv1.weight\n")
    with pytest.raises(ValueError):
        BitReader(weight_table=p).get_weight_channel_info()


def test_per_channel_cap_is_max_shift_limit_weight_per_channel():
    from tools.rewriter import BiasReWriter
    rw = BiasReWriter(None, None, None, None, None, None, max_shift_limit=12)
    feat, infeat = {"a": 4, "b": 6}, {"a": ["5"], "b": ["3", "3"]}
    # cap a: 12 - 5 + 4 = 11 (channels above, at and below the cap, and a zero channel's fallback bit); cap b: 12 - 3 + 6 = 15
    capped = rw.max_shift_limit_weight_per_channel(feat, infeat, {"a": [13, 11, 10, 7], "b": [15, 16, 2]})
    assert capped == {"a": [11, 11, 10, 7], "b": [15, 15, 2]}
    # every channel equal: exactly what the per-tensor cap gives
    for wbit in (9, 11, 14):
        _c, per_tensor = rw.max_shift_limit_weight(feat, infeat, {"a": wbit})
        assert rw.max_shift_limit_weight_per_channel(feat, infeat, {"a": [wbit] * 3}) == {"a": [per_tensor["a"]] * 3}
    assert BiasReWriter(None, None, None, None, None, None).max_shift_limit_weight_per_channel(feat, infeat, {"a": [20]}) == {"a": [20]}
    with pytest.raises(AssertionError):
        rw.max_shift_limit_weight_per_channel(feat, {"a": ["5", "6"]}, {"a": [1]})


def test_rescale_rows_is_the_per_tensor_rescale_row_by_row(tmp_path):
    from tools.rewriter import _rescale_file, rescale_rows
    rng = np.random.default_rng(5)
    q = rng.integers(-128, 128, (4, 3, 2, 2)).astype(np.int32)
    old, new = [9, 7, 7, 12], [9, 5, 3, 11]
    got = rescale_rows(q, old, new)
    for c in range(4):
        src, dst = str(tmp_path / "s.json"), str(tmp_path / "d.json")
        _write(src, json.dumps(q[c].tolist()))
        _rescale_file(src, dst, old[c], new[c])
        with open(dst) as fh:
            assert np.array_equal(np.array(json.load(fh), dtype=np.int8), got[c])


class _SmallNet(nn.Module):
    """Channels whose ranges differ by orders of magnitude, a zero channel, a dilated layer, a linear head."""

    def __init__(self):
        super(_SmallNet, self).__init__()
        from common.quantity import View
        self.conv1 = nn.Conv2d(3, 8, 3, padding=1)
        self.r1 = nn.ReLU(False)
        self.conv2 = nn.Conv2d(8, 8, 3, padding=2, dilation=2)
        self.r2 = nn.ReLU(False)
        self.pool = nn.AvgPool2d(8)
        self.view = View()
        self.fc = nn.Linear(8, 5)
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for m in (self.conv1, self.conv2, self.fc):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.3)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            self.conv1.weight[1] *= 2.0 ** -5
            self.conv1.weight[2] *= 2.0 ** -9
            self.conv1.weight[3] = 0.0
            self.conv2.weight[0] *= 64.0

    def forward(self, x):
        x = self.r1(self.conv1(x))
        x = self.r2(self.conv2(x))
        return self.fc(self.view(self.pool(x)))


def _oracle_row_max(self, tensors):
    from oracle import fq_oracle as orc
    return [np.array([orc.absmax(t[c].numpy()) for c in range(t.shape[0])], dtype=np.float32) for t in tensors]


@pytest.fixture(scope="module")
def calibrated(oracle):
    from tools import Quantity, Reconstruction

    class CpuQuantity(Quantity):
        collector_cls = OracleCollector
        quantizer_cls = OracleQuantizer
        _weight_row_max = _oracle_row_max

    out = {}
    with product_workdir(input_shape="1,3,8,8", device="cpu", max_cali_img_num=1) as tmp:
        model = _SmallNet().eval()
        q = CpuQuantity(model)
        q.activation_quantize(cases.calib_batches(2, (2, 3, 8, 8)))
        q.weight_quantize()
        wd = os.path.join(tmp, "test", "workdir")
        snapshot = {f: open(os.path.join(wd, f)).read() for f in ("weight.table", "feat.table")}
        per_tensor_files = sorted(os.listdir(os.path.join(wd, "weight")) + os.listdir(os.path.join(wd, "new_weight")))
        out["capped"] = q.weight_quantize_per_channel()
        out["unchanged"] = snapshot == {f: open(os.path.join(wd, f)).read() for f in snapshot} and per_tensor_files == sorted(
            os.listdir(os.path.join(wd, "weight")) + os.listdir(os.path.join(wd, "new_weight")))
        out["table"] = open(os.path.join(wd, "weight_channel.table")).read()
        out["json"] = {d: {f: json.load(open(os.path.join(wd, d, f))) for f in os.listdir(os.path.join(wd, d))}
                       for d in ("weight_channel", "new_weight_channel")}
        out["feat"] = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in snapshot["feat.table"].splitlines() if ln.strip()}
        out["weight_table"] = snapshot["weight.table"]
        rec = Reconstruction(model)
        out["info_pt"] = rec.get_quantity_information()
        out["info_pc"] = rec.get_quantity_information_per_channel()
        out["model"] = model
    return out


def test_weight_quantize_per_channel_table_grammar_and_order(calibrated):
    lines = calibrated["table"].splitlines()
    assert [ln.split()[0] for ln in lines] == [ln.split()[0] for ln in calibrated["weight_table"].splitlines()]
    for ln in lines:
        name, *bits = ln.split(" ")
        layer = name.rsplit(".", 1)[0]
        if name.endswith(".bias"):
            assert bits == [str(calibrated["feat"][layer][0])]                  # the output bit
        else:
            assert len(bits) == dict(calibrated["model"].named_modules())[layer].weight.shape[0]
            assert all(str(int(b)) == b for b in bits)
    assert calibrated["unchanged"], "the per-tensor files were touched"


def test_weight_quantize_per_channel_bits_and_json_match_numpy(calibrated):
    model, feat = calibrated["model"], calibrated["feat"]
    spread = False
    for layer in ("conv1", "conv2", "fc"):
        m = dict(model.named_modules())[layer]
        w = m.weight.detach()
        if isinstance(m, nn.Conv2d) and m.dilation != (1, 1):
            w = dilate_dense(w, m.dilation)
        wb0, tensor_bit = numpy_channel_bits(w.numpy())
        spread |= len(set(wb0)) > 2
        # the per-tensor bit is the largest channel's bit
        assert min(wb0) == tensor_bit
        cap = 12 - feat[layer][1] + feat[layer][0]
        wb = [min(b, cap) for b in wb0]
        assert calibrated["capped"][layer] == wb
        row = [ln for ln in calibrated["table"].splitlines() if ln.startswith(layer + ".weight ")][0]
        assert [int(v) for v in row.split()[1:]] == wb
        q0 = np.stack([np.clip(np.rint(w[c].numpy() * np.float32(2.0 ** b)), -128, 127) for c, b in enumerate(wb0)])
        assert np.array_equal(np.array(calibrated["json"]["weight_channel"][layer + ".weight.json"]), q0)
        resc = np.stack([np.around(q0[c].astype(np.float32) / 2 ** b0 * 2 ** b) for c, (b0, b) in enumerate(zip(wb0, wb))])
        resc = ((resc.astype(np.int64) + 128) % 256 - 128)
        assert np.array_equal(np.array(calibrated["json"]["new_weight_channel"][layer + ".weight.json"]), resc)
    # the zero channel takes the tensor's bit (then the cap)
    assert calibrated["capped"]["conv1"][3] == min(numpy_channel_bits(model.conv1.weight.detach().numpy())[1],
                                                    12 - feat["conv1"][1] + feat["conv1"][0])
    assert spread


def test_get_quantity_information_per_channel(calibrated):
    pt, pc = calibrated["info_pt"], calibrated["info_pc"]
    assert list(pt.keys()) == list(pc.keys())
    for name in pt:
        a, b = pt[name], pc[name]
        assert set(a) == set(b)
        for key in a:
            if key == "weight_bit" and a[key] is not None:
                assert b[key] == calibrated["capped"][name]
                assert min(b[key]) == a[key]                 # the largest channel's bit is the per-tensor bit
            elif key == "layer":
                assert a[key] is b[key]
            else:
                assert a[key] == b[key], (name, key)
        if a["weight_bit"] is not None:
            assert b["bias_bit"] == b["output_bit"]


def test_get_quantity_information_per_channel_from_hand_written_tables(oracle):
    from tools import Reconstruction
    with product_workdir(device="cpu") as tmp:
        wd = os.path.join(tmp, "test", "workdir")
        os.makedirs(wd)
        _write(os.path.join(wd, "feat.table"), "image 5\nconv1 3 5\nfc 2 3\n")
        _write(os.path.join(wd, "weight.table"), "conv1.weight 7\nconv1.bias 3\nfc.weight 6\nfc.bias 2\n")
        _write(os.path.join(wd, "weight_channel.table"), "conv1.weight 7 9 8\nconv1.bias 3\nfc.weight 6 6\nfc.bias 2\n")
        model = nn.Sequential()
        model.add_module("conv1", nn.Conv2d(2, 3, 1))
        model.add_module("fc", nn.Linear(3, 2))
        info = Reconstruction(model).get_quantity_information_per_channel()
        assert info["conv1"]["weight_bit"] == [7, 9, 8] and info["fc"]["weight_bit"] == [6, 6]
        assert (info["conv1"]["input_bit"], info["conv1"]["output_bit"], info["conv1"]["bias_bit"]) == (5, 3, 3)
        assert info["image"]["weight_bit"] is None and info["conv1"]["layer_type"] == "Conv2d"
        alt = os.path.join(wd, "other.table")
        _write(alt, "conv1.weight 1 2 3\nfc.weight 4 5\n")
        assert Reconstruction(model).get_quantity_information_per_channel(alt)["conv1"]["weight_bit"] == [1, 2, 3]

