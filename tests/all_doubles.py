"""Every oracle-backed double of common.quantity._native at once -- so that the CPU suite can run resident.enable() with all eight
switches (depthwise, concat, avgpool, grouped, relu6, flatten, shuffle, activations) on one model.

TEST INFRASTRUCTURE, as native_doubles.py: the product never imports this.  The existing modules form three chains that never meet
(native -> concat -> avgpool -> concat_n; native -> depthwise -> shuffle(+concat) -> activation; native -> depthwise -> grouped ->
relu6).  installed() enters all three, one inside the other, and copies nothing: each chain patches the names it knows, the one
entered later wins where two chains patch the same name, and leaving restores in reverse order.  The relu6 chain goes in LAST, because
it is the widest on every shared name: its four convolution doubles take `clip=`, and below them sit the depthwise module's
recon_epilogue (per-channel shifts) and the grouped doubles.  concat_i8_nhwc is concat_doubles' function in both chains that set it.
tests/test_mixed_plan_cpu.py shows which function each shared name ends up as.
"""
import contextlib

import activation_doubles
import concat_n_doubles
import relu6_doubles

CHAINS = (concat_n_doubles, activation_doubles, relu6_doubles)        # (order matters: see above)
# every entry point of _native that some chain patches besides native_doubles' own
NAMES = ("concat_i8_nhwc", "concat_n_i8_nhwc", "avgpool_i8_nhwc", "shuffle_i8_nhwc", "act_lut_i8_nhwc", "build_act_table",
         "pack_weight_dw", "dwconv2d_i8_resident", "recon_epilogue", "pack_weight_grouped", "gconv2d_i8_resident",
         "conv2d_i8_resident", "conv2d_i8_stem")


@contextlib.contextmanager
def installed():
    with contextlib.ExitStack() as stack:
        nat = None
        for chain in CHAINS:
            nat = stack.enter_context(chain.installed())
        yield nat
