"""Child process of tests/test_gpu_add_forms.py::test_the_streaming_1x1_kernel_s_add_epilogue_is_the_rule, started with
FQ_CONV_STREAM=1 (the library reads the switch once per process): the 1x1 pass-through layers of that module through
fq_conv2d_i8_add_resident and its _pcs sibling, every parameter set and both residual types, against tests/add_rule.py.  Prints
the kernel each layer's add launches ran and `add_forms_stream_child: OK`; any mismatch is an AssertionError."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "pytorch-quantity_amd", "quantity"), os.path.join(HERE, "golden"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    assert os.environ.get("FQ_CONV_STREAM") == "1", "start this with FQ_CONV_STREAM=1"
    import torch
    assert torch.cuda.is_available()
    from common.quantity import _native as nat
    import test_gpu_add_forms as t
    nat.lib()
    fused = t.build_fused(nat)
    for pcs in (False, True):
        names = t.conv_add_layers(nat, fused, pcs, t.STREAM_LAYERS)
        for layer in t.STREAM_LAYERS:
            want = t.DEFAULT_KERNELS[layer] if pcs else {"stream"}
            assert names[layer] and names[layer] <= want, (pcs, layer, names[layer])
        print("pcs" if pcs else "per_tensor", " ".join("+".join(sorted(names[layer])) for layer in t.STREAM_LAYERS))
    torch.cuda.synchronize()
    print("add_forms_stream_child: OK %d sets x %d layers x 2 entry points" % (len(fused["sets"]), len(t.STREAM_LAYERS)))


if __name__ == "__main__":
    main()
