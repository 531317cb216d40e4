"""One table for the size-limit tests: plain data and arithmetic, no torch, no library.

Every entry point of libfq_hip.so that indexes with 32 bits on the device refuses on the host what does not fit.  REFUSALS lists,
per guard, the first value it refuses (and, where the quantity is a product, one step above it): tests/test_size_guards_cpu.py
passes exactly these through ctypes and expects FQ_ERR_UNSUPPORTED.  GPU_CASES lists what tests/test_gpu_size_limits.py runs on the
device just BELOW the guards (or, for entry points that index with 64 bits and have no guard, beyond 2^31 bytes), with the bytes
each case allocates.  `args` are the entry point's integer arguments in the order ARGS names them.

Guards that no call can reach alone, because another one of the same entry point refuses every such shape first, are listed in
SHADOWED with the reason; they are kept in the C code as documentation of the kernel's own limit.
"""
import collections

GiB = 1 << 30

# entry point -> the names of `args`
ARGS = {
    "fq_conv1x1_f32": "N Cin H W Cout stride",
    "fq_conv1x1_sb_f32": "N Cin H W Cout stride",
    "fq_conv_kxk_f32": "N Cin H W Cout R S stride pad",
    "fq_conv1x1_add_f32": "N Cin H W Cout stride",
    "fq_conv1x1_sb_add_f32": "N Cin H W Cout stride",
    "fq_conv1x1_add_hist_f32": "N Cin H W Cout stride",
    "fq_conv1x1_sb_pack": "Cin Cout",
    "fq_conv_stem_f32": "N Cin H W Cout R S stride pad",
    "fq_conv3x3_wino_f32": "N Cin H W Cout",
    "fq_conv3x3_wino_f32_pack": "Cin Cout",
    "fq_dwconv_f32": "N C H W R S stride pad",
    "fq_gconv_f32": "N C H W K groups R S stride pad",
    "fq_maxpool2d_f32": "planes H W kh kw sh sw ph pw",
    "fq_bias_add_absmax_f32": "N C HW",
    "fq_bias_add_hist_f32": "N C HW",
    "fq_absmax_chan": "N C HW",                                      # one fq_chan_seg
    "fq_hist2048_chan": "N C HW",
    "fq_hist2048_chain_seg": "n",                                    # one chain of length 1
    "fq_quantize_i8_nhwc": "N C HW Cpad",
    "fq_dequant_nhwc_to_nchw": "N C HW Cpad",
    "fq_avgpool_global_nhwc": "N C HW Cpad",
    "fq_conv2d_i8": "N H W C K R S stride pad",                       # fp32 NCHW output only
    "fq_conv2d_i8_resident": "N H W C K R S stride pad",              # int8 NHWC output, Kpad = pad16(K)
    "fq_conv2d_i8_add_resident": "N H W C K R S stride pad",
    "fq_dwconv2d_i8_resident": "N H W C R S stride pad",              # Cpad = pad16(C)
    "fq_gconv2d_i8_resident": "N H W C K groups R S stride pad",
    "fq_avgpool_i8_nhwc": "N H W C kh kw sh sw ph pw",                # Cpad = pad16(C)
    "fq_concat_i8_nhwc": "N H W C0 Cpad0 up0 C1 Cpad1 up1",
    "fq_concat_n_i8_nhwc": "N H W C0 Cpad0 up0 C1 Cpad1 up1",
    "fq_block_tail_i8": "M C K3 C2",
    "fq_block_tail_proj_i8": "N H W C K3 C2 CP stride_p",
}


def pad16(c):
    return (c + 15) // 16 * 16


def out_size(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def prod(*v):
    r = 1
    for x in v:
        r *= x
    return r


# guard: "file: function"; quantity: what the guard bounds; limit: the first value it refuses; value: the quantity for `args`;
# exact: value == limit (else: the smallest value >= limit the entry point's other constraints let a call reach, or one step above)
Refusal = collections.namedtuple("Refusal", "id entry args guard quantity value limit exact")


def _r(id_, entry, args, guard, quantity, value, limit):
    assert len(args) == len(ARGS[entry].split()), id_
    return Refusal(id_, entry, tuple(args), guard, quantity, value, limit, value == limit)


C1 = "fq_conv1x1_f32.hip: conv_f32_launch"
C1A = "fq_conv1x1_f32.hip: conv_add_launch"
SB_LIMIT = (1 << 32) // 6 + 1                                         # the first Cin * Cout whose 6-byte pack does not end below 4 GiB
I31, I30, I29 = (1 << 31) - 1, (1 << 30) - 1, (1 << 29) - 1
POOL_STRIDE = 256 * 64 * 256                                          # fq_pool_f32.hip: kPoolMaxBlocks * kPoolBlock

REFUSALS = [
    # ---- float convolutions: 32-bit BYTE offsets, so 2^30 fp32 elements per tensor
    _r("c1_out", "fq_conv1x1_f32", (256, 16, 256, 256, 64, 1), C1, "N*Hout*Wout*Cout", prod(256, 256, 256, 64), 1 << 30),
    _r("c1_out_step", "fq_conv1x1_f32", (257, 16, 256, 256, 64, 1), C1, "N*Hout*Wout*Cout", prod(257, 256, 256, 64), 1 << 30),
    _r("c1_in", "fq_conv1x1_f32", (256, 64, 256, 256, 4, 1), C1, "N*Cin*Hin*Win", prod(256, 64, 256, 256), 1 << 30),
    _r("c1_in_step", "fq_conv1x1_f32", (257, 64, 256, 256, 4, 1), C1, "N*Cin*Hin*Win", prod(257, 64, 256, 256), 1 << 30),
    _r("c1_w", "fq_conv1x1_f32", (1, 32768, 1, 1, 32768, 1), C1, "R*S*Cin*Cout", 32768 * 32768, 1 << 30),
    _r("c1_w_step", "fq_conv1x1_f32", (1, 32768, 1, 1, 32772, 1), C1, "R*S*Cin*Cout", 32768 * 32772, 1 << 30),
    _r("c1_r101_512_b256", "fq_conv1x1_f32", (256, 64, 128, 128, 256, 1), C1, "N*Hout*Wout*Cout", prod(256, 128, 128, 256), 1 << 30),
    _r("kxk_w", "fq_conv_kxk_f32", (1, 16384, 3, 3, 7284, 3, 3, 1, 1), C1, "R*S*Cin*Cout", 9 * 16384 * 7284, 1 << 30),
    _r("kxk_out", "fq_conv_kxk_f32", (256, 16, 256, 256, 64, 3, 3, 1, 1), C1, "N*Hout*Wout*Cout", prod(256, 256, 256, 64), 1 << 30),
    _r("sb_w", "fq_conv1x1_sb_f32", (1, 32768, 1, 1, 21848, 1), C1, "Cin*Cout (6-byte pack)", 32768 * 21848, SB_LIMIT),
    _r("sb_w_step", "fq_conv1x1_sb_f32", (1, 32768, 1, 1, 21852, 1), C1, "Cin*Cout (6-byte pack)", 32768 * 21852, SB_LIMIT),
    _r("sb_pack", "fq_conv1x1_sb_pack", (32768, 21848), "fq_conv1x1_f32.hip: fq_conv1x1_sb_pack", "Cin*Cout (6-byte pack)",
       32768 * 21848, SB_LIMIT),
    _r("c1add_out", "fq_conv1x1_add_f32", (128, 16, 256, 256, 128, 1), C1A, "N*Hout*Wout*Cout", prod(128, 256, 256, 128), 1 << 30),
    _r("c1add_out_step", "fq_conv1x1_add_f32", (129, 16, 256, 256, 128, 1), C1A, "N*Hout*Wout*Cout", prod(129, 256, 256, 128), 1 << 30),
    _r("c1add_in", "fq_conv1x1_add_f32", (64, 256, 256, 256, 128, 1), C1A, "N*Cin*Hin*Win", prod(64, 256, 256, 256), 1 << 30),
    _r("c1add_w", "fq_conv1x1_add_f32", (1, 32768, 1, 1, 32768, 1), C1A, "Cin*Cout", 32768 * 32768, 1 << 30),
    _r("c1add_hist_out", "fq_conv1x1_add_hist_f32", (128, 16, 256, 256, 128, 1), C1A, "N*Hout*Wout*Cout", prod(128, 256, 256, 128), 1 << 30),
    _r("sbadd_w", "fq_conv1x1_sb_add_f32", (1, 32768, 1, 1, 21888, 1), C1A, "Cin*Cout (6-byte pack)", 32768 * 21888, SB_LIMIT),
    _r("stem_out", "fq_conv_stem_f32", (256, 3, 512, 512, 64, 7, 7, 2, 3), "fq_conv_stem_f32.hip: stem_launch", "N*Cout*Hout*Wout",
       prod(256, 64, 256, 256), 1 << 30),
    _r("stem_out_step", "fq_conv_stem_f32", (257, 3, 512, 512, 64, 7, 7, 2, 3), "fq_conv_stem_f32.hip: stem_launch", "N*Cout*Hout*Wout",
       prod(257, 64, 256, 256), 1 << 30),
    _r("stem_in", "fq_conv_stem_f32", (342, 3, 1024, 1024, 4, 7, 7, 2, 3), "fq_conv_stem_f32.hip: stem_launch", "N*Cin*H*W",
       prod(342, 3, 1024, 1024), 1 << 30),
    _r("wino_out", "fq_conv3x3_wino_f32", (128, 8, 64, 64, 1024), "fq_conv_wino_f32.hip: wino_shape_ok", "N*Cout*H*W*4",
       prod(128, 1024, 64, 64, 4), 1 << 31),
    _r("wino_in", "fq_conv3x3_wino_f32", (128, 1024, 64, 64, 64), "fq_conv_wino_f32.hip: wino_shape_ok", "N*Cin*H*W*4",
       prod(128, 1024, 64, 64, 4), 1 << 31),
    _r("wino_w", "fq_conv3x3_wino_f32", (1, 4096, 2, 2, 8192), "fq_conv_wino_f32.hip: wino_shape_ok", "Cin*Cout*64", 4096 * 8192 * 64, 1 << 31),
    _r("wino_pack", "fq_conv3x3_wino_f32_pack", (4096, 8192), "fq_conv_wino_f32.hip: fq_conv3x3_wino_f32_pack", "Cin*Cout*64",
       4096 * 8192 * 64, 1 << 31),
    _r("dwf_in", "fq_dwconv_f32", (256, 64, 256, 256, 3, 3, 2, 1), "fq_dwconv_f32.hip: dwf_dispatch", "N*C*H*W", prod(256, 64, 256, 256), 1 << 30),
    _r("dwf_in_step", "fq_dwconv_f32", (257, 64, 256, 256, 3, 3, 2, 1), "fq_dwconv_f32.hip: dwf_dispatch", "N*C*H*W", prod(257, 64, 256, 256), 1 << 30),
    _r("dwf_out", "fq_dwconv_f32", (253, 64, 256, 256, 3, 3, 1, 2), "fq_dwconv_f32.hip: dwf_dispatch", "N*C*Ho*Wo", prod(253, 64, 258, 258), 1 << 30),
    _r("gf_in", "fq_gconv_f32", (256, 64, 256, 256, 8, 2, 1, 1, 1, 0), "fq_gconv_f32.hip: gf_dispatch", "N*C*H*W", prod(256, 64, 256, 256), 1 << 30),
    _r("gf_out", "fq_gconv_f32", (256, 8, 256, 256, 64, 2, 1, 1, 1, 0), "fq_gconv_f32.hip: gf_dispatch", "N*K*Ho*Wo", prod(256, 64, 256, 256), 1 << 30),
    _r("gf_out_step", "fq_gconv_f32", (257, 8, 256, 256, 64, 2, 1, 1, 1, 0), "fq_gconv_f32.hip: gf_dispatch", "N*K*Ho*Wo", prod(257, 64, 256, 256), 1 << 30),
    _r("gf_w", "fq_gconv_f32", (1, 29128 * 64, 1, 1, 29128 * 64, 29128, 3, 3, 1, 1), "fq_gconv_f32.hip: gf_dispatch", "K*(C/groups)*R*S",
       prod(29128 * 64, 64, 9), 1 << 30),
    # ---- float pooling and element-wise producers: 32-bit element indices
    _r("pool_wrap", "fq_maxpool2d_f32", (65472, 256, 256, 1, 1, 1, 1, 0, 0), "fq_pool_f32.hip: fq_maxpool2d_f32", "outputs + grid stride",
       prod(65472, 256, 256) + POOL_STRIDE, 1 << 32),
    _r("pool_2_32", "fq_maxpool2d_f32", (65536, 256, 256, 1, 1, 1, 1, 0, 0), "fq_pool_f32.hip: fq_maxpool2d_f32", "outputs + grid stride",
       (1 << 32) + POOL_STRIDE, 1 << 32),
    _r("pool_in", "fq_maxpool2d_f32", (65537, 65535, 1, 1, 1, 65535, 1, 0, 0), "fq_pool_f32.hip: fq_maxpool2d_f32", "planes*H*W",
       65537 * 65535, (1 << 32) - 1),
    _r("pool_plane", "fq_maxpool2d_f32", (1, 65536, 32768, 1, 1, 65536, 32768, 0, 0), "fq_pool_f32.hip: fq_maxpool2d_f32", "H*W",
       65536 * 32768, 1 << 31),
    _r("bias_absmax", "fq_bias_add_absmax_f32", (65537, 65535, 1), "fq_ops.hip: fq_bias_add_absmax_f32", "N*C*HW", 65537 * 65535, (1 << 32) - 1),
    _r("bias_absmax_step", "fq_bias_add_absmax_f32", (65537, 65536, 1), "fq_ops.hip: fq_bias_add_absmax_f32", "N*C*HW", 65537 * 65536, (1 << 32) - 1),
    _r("bias_hist", "fq_bias_add_hist_f32", (65537, 65535, 1), "fq_ops.hip: fq_bias_add_hist_f32", "N*C*HW", 65537 * 65535, (1 << 32) - 1),
    _r("bias_hist_step", "fq_bias_add_hist_f32", (65537, 65536, 1), "fq_ops.hip: fq_bias_add_hist_f32", "N*C*HW", 65537 * 65536, (1 << 32) - 1),
    # ---- per-channel statistics: fq_chan_seg.HW is 64 bits wide and narrowed to 32 in the kernel's table; the chain histogram
    #      numbers its 16 KB chunks (1024 vectors of four floats) with 32 bits
    _r("absmax_chan_hw", "fq_absmax_chan", (1, 1, 1 << 31), "fq_calib.hip: for_each_chan_chunk", "HW", 1 << 31, 1 << 31),
    _r("hist_chan_hw", "fq_hist2048_chan", (1, 1, 1 << 31), "fq_calib.hip: for_each_chan_chunk", "HW", 1 << 31, 1 << 31),
    _r("chain_chunks", "fq_hist2048_chain_seg", (4 * (I31 * 1024 + 1),), "fq_calib.hip: launch_chain", "ceil(n / 4 / 1024)", 1 << 31, 1 << 31),
    # ---- layout changes: the image index is a grid dimension
    _r("quantize_n", "fq_quantize_i8_nhwc", (65536, 16, 2, 16), "fq_conv_i8.hip: fq_quantize_i8_nhwc", "N (general form)", 65536, 65536),
    _r("dequant_n", "fq_dequant_nhwc_to_nchw", (65536, 16, 2, 16), "fq_resident.hip: fq_dequant_nhwc_to_nchw", "N", 65536, 65536),
    _r("avgpool_global_hw", "fq_avgpool_global_nhwc", (1, 16, 512, 16), "fq_resident.hip: fq_avgpool_global_nhwc", "HW*32768", 512 * 32768, 1 << 24),
    # ---- dense int8 convolution: signed 32-bit byte offsets into x and w, element offsets into the outputs
    _r("i8_x", "fq_conv2d_i8_resident", (512, 256, 256, 64, 16, 1, 1, 1, 0), "fq_conv_i8.hip: conv2d_i8_dispatch", "N*H*W*C",
       prod(512, 256, 256, 64), I31),
    _r("i8_x_3x3", "fq_conv2d_i8", (512, 256, 256, 64, 16, 3, 3, 2, 1), "fq_conv_i8.hip: conv2d_i8_dispatch", "N*H*W*C",
       prod(512, 256, 256, 64), I31),
    _r("i8_w", "fq_conv2d_i8_resident", (1, 1, 1, 65536, 32768, 1, 1, 1, 0), "fq_conv_i8.hip: conv2d_i8_dispatch", "K*R*S*C", 32768 * 65536, I31),
    _r("i8_kpq", "fq_conv2d_i8", (1, 1024, 1024, 16, 512, 1, 1, 1, 0), "fq_conv_i8.hip: conv2d_i8_dispatch", "K*P*Q", 512 * 1024 * 1024, I29 + 1),
    _r("i8_kpq_step", "fq_conv2d_i8", (1, 1024, 1025, 16, 512, 1, 1, 1, 0), "fq_conv_i8.hip: conv2d_i8_dispatch", "K*P*Q", 512 * 1024 * 1025, I29 + 1),
    _r("i8_mkpad", "fq_conv2d_i8_resident", (64, 1024, 1024, 16, 16, 1, 1, 1, 0), "fq_conv_i8.hip: conv2d_i8_dispatch", "M*Kpad",
       prod(64, 1024, 1024, 16), I30),
    _r("i8_mkpad_r101", "fq_conv2d_i8_resident", (79, 256, 256, 16, 200, 1, 1, 1, 0), "fq_conv_i8.hip: conv2d_i8_dispatch", "M*Kpad",
       prod(79, 256, 256, 208), I30),
    _r("i8_mkpad_add", "fq_conv2d_i8_add_resident", (64, 1024, 1024, 16, 16, 1, 1, 1, 0), "fq_conv_i8.hip: conv2d_i8_dispatch", "M*Kpad",
       prod(64, 1024, 1024, 16), I30),
    # ---- the other int8 kernels
    _r("dwi_in", "fq_dwconv2d_i8_resident", (512, 256, 256, 64, 3, 3, 2, 1), "fq_dwconv_i8.hip: dwconv_dispatch", "N*H*W*Cpad",
       prod(512, 256, 256, 64), I31),
    _r("dwi_out", "fq_dwconv2d_i8_resident", (256, 256, 256, 64, 3, 3, 1, 1), "fq_dwconv_i8.hip: dwconv_dispatch", "N*P*Q*Cpad",
       prod(256, 256, 256, 64), I30),
    _r("dwi_cpad", "fq_dwconv2d_i8_resident", (1, 3, 3, 65552, 3, 3, 1, 1), "fq_dwconv_i8.hip: dwconv_dispatch", "Cpad", 65552, 65537),
    _r("gci_in", "fq_gconv2d_i8_resident", (512, 256, 256, 64, 64, 2, 1, 1, 2, 0), "fq_gconv_i8.hip: gconv_dispatch", "N*H*W*Cpad",
       prod(512, 256, 256, 64), I31),
    _r("gci_out", "fq_gconv2d_i8_resident", (256, 256, 256, 64, 64, 2, 1, 1, 1, 0), "fq_gconv_i8.hip: gconv_dispatch", "N*P*Q*Kpad",
       prod(256, 256, 256, 64), I30),
    _r("avgi_in", "fq_avgpool_i8_nhwc", (512, 256, 256, 64, 3, 3, 2, 2, 1, 1), "fq_avgpool_i8.hip: fq_avgpool_i8_nhwc", "N*H*W*Cpad",
       prod(512, 256, 256, 64), I31),
    _r("avgi_out", "fq_avgpool_i8_nhwc", (509, 256, 256, 64, 2, 2, 1, 1, 1, 1), "fq_avgpool_i8.hip: fq_avgpool_i8_nhwc", "N*P*Q*Cpad",
       prod(509, 257, 257, 64), I31),
    _r("cat_out", "fq_concat_i8_nhwc", (512, 256, 256, 32, 32, 1, 32, 32, 1), "fq_concat_i8.hip: fq_concat_i8_nhwc", "N*H*W*Cpad_out",
       prod(512, 256, 256, 64), I31),
    _r("cat_src", "fq_concat_i8_nhwc", (32, 256, 256, 1, 1024, 1, 1, 16, 1), "fq_concat_i8.hip: fq_concat_i8_nhwc", "N*(H/up)*(W/up)*Cpad_src",
       prod(32, 256, 256, 1024), I31),
    _r("catn_out", "fq_concat_n_i8_nhwc", (512, 256, 256, 32, 32, 1, 32, 32, 1), "fq_concat_i8.hip: fq_concat_n_i8_nhwc", "N*H*W*Cpad_out",
       prod(512, 256, 256, 64), I31),
    _r("catn_src", "fq_concat_n_i8_nhwc", (32, 256, 256, 1, 1024, 1, 1, 16, 1), "fq_concat_i8.hip: fq_concat_n_i8_nhwc",
       "N*(H/up)*(W/up)*Cpad_src", prod(32, 256, 256, 1024), I31),
    _r("bt_mk3", "fq_block_tail_i8", (1 << 23, 64, 128, 0), "fq_block_tail_i8.hip: block_tail_dispatch", "M*K3", (1 << 23) * 128, I30),
    _r("btp_mk3", "fq_block_tail_proj_i8", (128, 256, 256, 64, 128, 0, 64, 1), "fq_block_tail_i8.hip: block_tail_proj_dispatch", "M*K3",
       prod(128, 256, 256, 128), I30),
]

# the smallest step of a quantity that its entry point's divisibility rules allow: value - limit of a non-exact row stays below it
REACH = {
    "kxk_w": 9 * 16384 * 4, "sb_w": 32768 * 4, "sb_pack": 32768 * 4, "sbadd_w": 32768 * 128, "stem_in": 3 * 1024 * 1024,
    "dwf_out": 64 * 258 * 258, "gf_w": 64 * 64 * 9, "pool_2_32": POOL_STRIDE + 1, "i8_x": 16, "i8_x_3x3": 16, "i8_w": 16,
    "i8_mkpad": 16, "i8_mkpad_add": 16, "i8_mkpad_r101": 208 * 79 * 511, "dwi_in": 16, "dwi_out": 16, "dwi_cpad": 16, "gci_in": 16,
    "gci_out": 16, "avgi_in": 16, "avgi_out": 64 * 257 * 257, "cat_out": 16, "cat_src": 16, "catn_out": 16, "catn_src": 16,
    "bt_mk3": 128, "btp_mk3": 128,
}

SHADOWED = [
    ("fq_conv1x1_f32.hip: conv_f32_launch / conv_add_launch", "cols >= 0xffffff00",
     "Cout >= 4, so such a call has more than 2^30 outputs and the output guard of the same line refuses it"),
    ("fq_conv_stem_f32.hip: stem_launch", "tiles >= 2^31 - 1", "a tile holds 128 outputs per channel: the output guard refuses first"),
    ("fq_conv_wino_f32.hip: wino_shape_ok", "tiles >= 2^30, work >= 2^31", "a tile covers four input pixels: the input-bytes guard refuses first"),
    ("fq_conv_i8.hip: conv2d_i8_dispatch", "R*S*C/16 > 2^31 - 1", "K >= 1: K*R*S*C >= 2^31 - 1 of the next line refuses every such call"),
    ("fq_conv_i8.hip: conv2d_i8_dispatch", "M > 2^31 - 1", "C >= 16 bytes per pixel and a window per output: refused together with N*H*W*C"),
    ("fq_block_tail_i8.hip: block_tail_dispatch", "M*C >= 2^31 - 1", "C <= 256 <= 2 * K3: M*K3 >= 2^30 - 1 refuses first"),
    ("fq_block_tail_i8.hip: block_tail_proj_dispatch", "M*C, Mp*CP >= 2^31 - 1", "C = CP = 64, Mp <= 4 M, K3 >= 128: M*K3 refuses first"),
    ("fq_stem.hip: stem_dispatch", "ntiles > 2^31 - 1", "64-bit addresses throughout; 2^31 tiles of 128 pixels are 16 TB of output"),
]


# ---- what runs on the GPU --------------------------------------------------------------------------------------------------
# kind "top": value >= 98 % of the guard's limit (the last admitted values), every tiled dimension ragged;
# kind "bit31": the entry point has no guard of this kind (64-bit indices) or the row is about the byte offset: some operand is
#               larger than 2^31 bytes.  big_bytes: that operand's size.  peak_bytes: everything the case holds at once on the
#               device, the chunk of the reference included.
GpuCase = collections.namedtuple("GpuCase", "id entry args kind guard quantity value limit big_bytes peak_bytes ragged")

REF_CHUNK = 3 * GiB // 2                                              # what a case may hold for one chunk of its reference


def _g(id_, entry, args, kind, guard, quantity, value, limit, big_bytes, tensors_bytes, ragged=()):
    return GpuCase(id_, entry, tuple(args), kind, guard, quantity, value, limit, big_bytes, tensors_bytes + REF_CHUNK, tuple(ragged))


N_FLAT = (1 << 31) + 4099                                             # a scalar tail of 3 behind the 16-byte vectors


def _c1(n, cin, h, w, cout, copies=1):
    """bytes of x, w, bias and `copies` outputs of a float convolution at stride 1"""
    return 4 * (n * cin * h * w + cin * cout + cout + copies * n * cout * h * w)


GPU_CASES = [
    # float convolutions (limit 2^30 elements)
    _g("c1_bit31", "fq_conv1x1_f32", (36, 16, 128, 128, 1024, 1), "bit31", C1, "y bytes", 4 * prod(36, 128, 128, 1024), None,
       4 * prod(36, 128, 128, 1024), _c1(36, 16, 128, 128, 1024)),
    _g("c1_top", "fq_conv1x1_f32", (63, 16, 127, 129, 1036, 1), "top", C1, "N*Hout*Wout*Cout", prod(63, 127, 129, 1036), 1 << 30,
       4 * prod(63, 127, 129, 1036), _c1(63, 16, 127, 129, 1036, copies=2) + 6 * 16 * 1036,
       ragged=(("cols", 63 * 127 * 129, 128), ("Cout", 1036, 128))),
    _g("c1_top_ktail", "fq_conv1x1_f32", (63, 20, 127, 129, 1036, 1), "top", C1, "N*Hout*Wout*Cout", prod(63, 127, 129, 1036), 1 << 30,
       4 * prod(63, 127, 129, 1036), _c1(63, 20, 127, 129, 1036),
       ragged=(("cols", 63 * 127 * 129, 128), ("Cout", 1036, 128), ("Cin", 20, 16))),
    _g("c1_in_top", "fq_conv1x1_f32", (63, 1024, 128, 128, 8, 1), "top", C1, "N*Cin*Hin*Win", prod(63, 1024, 128, 128), 1 << 30,
       4 * prod(63, 1024, 128, 128), _c1(63, 1024, 128, 128, 8), ragged=(("Cout", 8, 128),)),
    _g("kxk_top", "fq_conv_kxk_f32", (63, 16, 127, 129, 1036, 3, 3, 1, 1), "top", C1, "N*Hout*Wout*Cout", prod(63, 127, 129, 1036), 1 << 30,
       4 * prod(63, 127, 129, 1036), _c1(63, 16, 127, 129, 1036) + 4 * 8 * 16 * 1036,
       ragged=(("cols", 63 * 127 * 129, 128), ("Cout", 1036, 128))),
    _g("c1add_top", "fq_conv1x1_add_f32", (63, 16, 127, 129, 1024, 1), "top", C1A, "N*Hout*Wout*Cout", prod(63, 127, 129, 1024), 1 << 30,
       4 * prod(63, 127, 129, 1024), _c1(63, 16, 127, 129, 1024, copies=4) + 6 * 16 * 1024, ragged=(("cols", 63 * 127 * 129, 128),)),
    # Winograd 3x3: the smallest Cin it takes, odd planes, y at 99.98 % of 2^31 bytes (no geometry header: read, not walked)
    _g("wino_top", "fq_conv3x3_wino_f32", (520, 8, 127, 127, 64), "top", "fq_conv_wino_f32.hip: wino_shape_ok", "N*Cout*H*W*4",
       4 * prod(520, 64, 127, 127), 1 << 31, 4 * prod(520, 64, 127, 127), 4 * prod(520, 8, 127, 127) + 8 * prod(520, 64, 127, 127),
       ragged=(("H", 127, 2), ("W", 127, 2))),
    # depthwise and grouped fp32 (32-bit element offsets, limit 2^30 elements): odd planes, stride 1
    _g("dwf_top", "fq_dwconv_f32", (128, 520, 127, 127, 3, 3, 1, 1), "top", "fq_dwconv_f32.hip: dwf_dispatch", "N*C*Ho*Wo",
       prod(128, 520, 127, 127), 1 << 30, 4 * prod(128, 520, 127, 127), 12 * prod(128, 520, 127, 127),
       ragged=(("Wo", 127, 4), ("Ho", 127, 16))),
    _g("gf_top", "fq_gconv_f32", (1109, 20, 127, 127, 60, 5, 3, 3, 1, 1), "top", "fq_gconv_f32.hip: gf_dispatch", "N*K*Ho*Wo",
       prod(1109, 60, 127, 127), 1 << 30, 4 * prod(1109, 60, 127, 127), 4 * prod(1109, 20, 127, 127) + 8 * prod(1109, 60, 127, 127),
       ragged=(("Wo", 127, 4), ("Cgo", 12, 8))),
    _g("stem_f32_r101_512_b255", "fq_conv_stem_f32", (255, 3, 512, 512, 64, 7, 7, 2, 3), "top", "fq_conv_stem_f32.hip: stem_launch",
       "N*Cout*Hout*Wout", prod(255, 64, 256, 256), 1 << 30, 4 * prod(255, 64, 256, 256),
       4 * (prod(255, 3, 512, 512) + 2 * prod(255, 64, 256, 256))),
    # float pooling and element-wise producers
    _g("pool_quad", "fq_maxpool2d_f32", (8200, 512, 512, 3, 3, 2, 2, 1, 1), "bit31", "fq_pool_f32.hip: fq_maxpool2d_f32", "planes*H*W",
       prod(8200, 512, 512), (1 << 32) - 1, 4 * prod(8200, 512, 512), 4 * (prod(8200, 512, 512) + prod(8200, 256, 256))),
    _g("pool_generic", "fq_maxpool2d_f32", (4100, 724, 724, 2, 2, 2, 2, 0, 0), "bit31", "fq_pool_f32.hip: fq_maxpool2d_f32", "planes*H*W",
       prod(4100, 724, 724), (1 << 32) - 1, 4 * prod(4100, 724, 724), 4 * (prod(4100, 724, 724) + prod(4100, 362, 362))),
    _g("quandequan_flat", "fq_quandequan_f32", (N_FLAT,), "bit31", "fq_ops.hip: launch_unary", "n", N_FLAT, None, 4 * N_FLAT, 8 * N_FLAT),
    _g("add_sat_flat", "fq_add_sat_f32", (N_FLAT,), "bit31", "fq_ops.hip: fq_add_sat_f32", "n", N_FLAT, None, 4 * N_FLAT, 12 * N_FLAT),
    _g("bias_absmax_vec", "fq_bias_add_absmax_f32", (67, 71, 451588), "bit31", "fq_ops.hip: fq_bias_add_absmax_f32", "N*C*HW",
       prod(67, 71, 451588), (1 << 32) - 1, 4 * prod(67, 71, 451588), 8 * prod(67, 71, 451588)),
    _g("bias_absmax_odd", "fq_bias_add_absmax_f32", (67, 71, 451589), "bit31", "fq_ops.hip: fq_bias_add_absmax_f32", "N*C*HW",
       prod(67, 71, 451589), (1 << 32) - 1, 4 * prod(67, 71, 451589), 8 * prod(67, 71, 451589)),
    _g("bias_hist_vec", "fq_bias_add_hist_f32", (67, 71, 451588), "bit31", "fq_ops.hip: fq_bias_add_hist_f32", "N*C*HW",
       prod(67, 71, 451588), (1 << 32) - 1, 4 * prod(67, 71, 451588), 8 * prod(67, 71, 451588)),
    _g("bias_hist_odd", "fq_bias_add_hist_f32", (67, 71, 451589), "bit31", "fq_ops.hip: fq_bias_add_hist_f32", "N*C*HW",
       prod(67, 71, 451589), (1 << 32) - 1, 4 * prod(67, 71, 451589), 8 * prod(67, 71, 451589)),
    _g("add_absmax_flat", "fq_add_absmax_f32", (N_FLAT,), "bit31", "fq_ops.hip: fq_add_absmax_f32", "n", N_FLAT, None, 4 * N_FLAT, 12 * N_FLAT),
    _g("add_hist_flat", "fq_add_hist_f32", (N_FLAT,), "bit31", "fq_ops.hip: fq_add_hist_f32", "n", N_FLAT, None, 4 * N_FLAT, 12 * N_FLAT),
    _g("absmax_seg_flat", "fq_absmax_seg", (N_FLAT,), "bit31", "fq_calib.hip: for_each_chunk", "n", N_FLAT, None, 4 * N_FLAT, 4 * N_FLAT),
    _g("hist_seg_flat", "fq_hist2048_seg", (N_FLAT,), "bit31", "fq_calib.hip: for_each_chunk", "n", N_FLAT, None, 4 * N_FLAT, 4 * N_FLAT),
    # dense int8 convolution, the register-staged tile kernel (conv2d_i8_kernel): signed 32-bit byte offsets into x, 32-bit element
    # offsets into the [M][Kpad] outputs, a 64-bit base per lane for the fp32 NCHW output
    _g("i8_in_top_k16", "fq_conv2d_i8_resident", (255, 256, 256, 128, 16, 1, 1, 1, 0), "top", "fq_conv_i8.hip: conv2d_i8_dispatch",
       "N*H*W*C", prod(255, 256, 256, 128), I31, prod(255, 256, 256, 128), prod(255, 256, 256, 128) + 5 * prod(255, 256, 256, 16),
       ragged=(("K", 16, 64),)),
    _g("i8_out_top", "fq_conv2d_i8_resident", (79, 255, 255, 16, 200, 1, 1, 1, 0), "top", "fq_conv_i8.hip: conv2d_i8_dispatch",
       "M*Kpad", prod(79, 255, 255, 208), I30, 4 * prod(79, 255, 255, 200),
       prod(79, 255, 255, 16) + 4 * prod(79, 255, 255, 200) + 6 * prod(79, 255, 255, 208),
       ragged=(("M", 79 * 255 * 255, 128), ("K", 200, 128), ("K (Kpad != K)", 200, 16))),
    # ... and the other kernels behind the dispatcher at the input's top: the C % 128 == 0 path of the tile kernel (K = 64), the
    # LDS-DMA kernel (3x3 stride 2) and the stationary-weight 64-channel kernel.  That last one takes planes up to 66 pixels wide only
    # (its input slab of 130 + 2 W pixel rows must leave room for two workgroups per CU), so its row is 8454 images of 63 x 63, and
    # with M * Kpad beyond 2^30 only its fp32 output is admitted
    _g("i8_in_top_k64", "fq_conv2d_i8_resident", (255, 256, 256, 128, 64, 1, 1, 1, 0), "top", "fq_conv_i8.hip: conv2d_i8_dispatch",
       "N*H*W*C", prod(255, 256, 256, 128), I31, prod(255, 256, 256, 128), prod(255, 256, 256, 128) + 6 * prod(255, 256, 256, 64),
       ragged=(("K", 64, 128),)),
    _g("i8_in_top_3x3s2", "fq_conv2d_i8_resident", (255, 256, 256, 128, 64, 3, 3, 2, 1), "top", "fq_conv_i8.hip: conv2d_i8_dispatch",
       "N*H*W*C", prod(255, 256, 256, 128), I31, prod(255, 256, 256, 128), prod(255, 256, 256, 128) + 5 * prod(255, 128, 128, 64),
       ragged=(("K", 64, 128),)),
    _g("i8_in_top_c64", "fq_conv2d_i8", (8454, 63, 63, 64, 64, 3, 3, 1, 1), "top", "fq_conv_i8.hip: conv2d_i8_dispatch",
       "N*H*W*C", prod(8454, 63, 63, 64), I31, 4 * prod(8454, 63, 63, 64), 5 * prod(8454, 63, 63, 64),
       ragged=(("M", 8454 * 63 * 63, 128), ("plane", 63 * 63, 128))),
    _g("i8_f32_4gib", "fq_conv2d_i8", (300, 240, 240, 16, 64, 1, 1, 1, 0), "bit31", "fq_conv_i8.hip: conv2d_i8_dispatch", "y bytes",
       4 * prod(300, 64, 240, 240), None, 4 * prod(300, 64, 240, 240), prod(300, 240, 240, 16) + 4 * prod(300, 64, 240, 240)),
    # the two concatenation kernels, general family (C0 % 16 != 0: dword and byte-shifted chunks, one that straddles two sources), the
    # first source upsampled by 2; args: N H W then (C, up) per source.  WALKER_ROWS names the walker call that precedes the row
    _g("cat_top", "fq_concat_i8_nhwc", (520, 254, 254, 20, 2, 44, 1), "top", "fq_concat_i8.hip: fq_concat_i8_nhwc", "N*H*W*Cpad_out",
       prod(520, 254, 254, 64), I31, prod(520, 254, 254, 64), prod(520, 254, 254, 64) + prod(520, 127, 127, 32) + prod(520, 254, 254, 48),
       ragged=(("C0", 20, 16),)),
    _g("catn_top", "fq_concat_n_i8_nhwc", (520, 254, 254, 20, 2, 3, 1, 41, 1), "top", "fq_concat_i8.hip: fq_concat_n_i8_nhwc",
       "N*H*W*Cpad_out", prod(520, 254, 254, 64), I31, prod(520, 254, 254, 64),
       prod(520, 254, 254, 64) + prod(520, 127, 127, 32) + prod(520, 254, 254, 16) + prod(520, 254, 254, 48),
       ragged=(("C0", 20, 16), ("C0 + C1", 23, 16))),
    # the block tails (conv3 + NewAdd + the next conv1 in one kernel): 32-bit element offsets into the [M][K3] tensors; args N H W C K3 C2
    # (+ CP stride_p Hp Wp for the projection form, whose shortcut is computed in the kernel from a 125 x 125 plane at stride 2).
    # Declared bytes: x, the int16 shortcut and sum, the int8 sum, q1, and three more [M][K3] bytes per pixel of headroom -- the
    # allocator's peak was 7.8 GiB where the operands alone are 5.5
    _g("bt_top", "fq_block_tail_i8", (1056, 63, 63, 64, 256, 64), "top", "fq_block_tail_i8.hip: block_tail_dispatch", "M*K3",
       prod(1056, 63, 63, 256), I30, 2 * prod(1056, 63, 63, 256), prod(1056, 63, 63) * (64 + 8 * 256 + 64),
       ragged=(("M", 1056 * 63 * 63, 128),)),
    _g("btp_top", "fq_block_tail_proj_i8", (1056, 63, 63, 64, 256, 64, 64, 2, 125, 125), "top", "fq_block_tail_i8.hip: block_tail_proj_dispatch",
       "M*K3", prod(1056, 63, 63, 256), I30, 2 * prod(1056, 63, 63, 256),
       prod(1056, 63, 63) * (64 + 6 * 256 + 64) + prod(1056, 125, 125, 64), ragged=(("M", 1056 * 63 * 63, 128), ("Hp", 125, 2))),
    # depthwise int8: 32-bit element offsets into both activations; args N H W C R S stride pad (Cpad = 32: 13 padding channels)
    _g("dwi_top", "fq_dwconv2d_i8_resident", (2080, 127, 127, 19, 3, 3, 1, 1), "top", "fq_dwconv_i8.hip: dwconv_dispatch", "N*P*Q*Cpad",
       prod(2080, 127, 127, 32), I30, prod(2080, 127, 127, 32), 2 * prod(2080, 127, 127, 32),
       ragged=(("P", 127, 4), ("Q", 127, 4), ("C", 19, 16))),
    # grouped int8: 5 groups of 4 -> 12 channels (K = 60: one padding quad, Cpad 32, Kpad 64); args N H W C K groups R S stride pad
    _g("gci_top", "fq_gconv2d_i8_resident", (1040, 127, 127, 20, 60, 5, 3, 3, 1, 1), "top", "fq_gconv_i8.hip: gconv_dispatch", "N*P*Q*Kpad",
       prod(1040, 127, 127, 64), I30, prod(1040, 127, 127, 64), prod(1040, 127, 127, 64) + prod(1040, 127, 127, 32),
       ragged=(("Q", 127, 4), ("K", 60, 16), ("C", 20, 16))),
    # windowed int8 average pool: 32-bit byte offsets into the source, a 32-bit chunk index; args N H W C kh kw sh sw ph pw
    _g("avgi_top", "fq_avgpool_i8_nhwc", (4160, 127, 127, 19, 3, 3, 1, 1, 1, 1), "top", "fq_avgpool_i8.hip: fq_avgpool_i8_nhwc",
       "N*H*W*Cpad", prod(4160, 127, 127, 32), I31, prod(4160, 127, 127, 32), 2 * prod(4160, 127, 127, 32), ragged=(("C", 19, 16),)),
    # int8 kernels with 64-bit indices: an operand above 2^31 bytes
    _g("stem_i8_b520", "fq_conv2d_i8_stem", (520, 3, 512, 512, 64, 7, 7, 2, 3), "bit31", "fq_stem.hip: stem_dispatch", "q bytes",
       prod(520, 256, 256, 64), None, prod(520, 256, 256, 64), 4 * prod(520, 3, 512, 512) + prod(520, 256, 256, 64)),
    _g("maxpool_i8_banded", "fq_maxpool_i8_nhwc", (1051, 254, 126, 64, 3, 3, 2, 2, 1, 1), "bit31", "fq_resident.hip: fq_maxpool_i8_nhwc",
       "x bytes", prod(1051, 254, 126, 64), None, prod(1051, 254, 126, 64), prod(1051, 254, 126, 64) + prod(1051, 127, 63, 64)),
    _g("maxpool_i8_generic", "fq_maxpool_i8_nhwc", (529, 253, 251, 64, 2, 2, 2, 2, 0, 0), "bit31", "fq_resident.hip: fq_maxpool_i8_nhwc",
       "x bytes", prod(529, 253, 251, 64), None, prod(529, 253, 251, 64), prod(529, 253, 251, 64) + prod(529, 126, 125, 64)),
    _g("add_resident_i16", "fq_add_resident", ((1 << 30) + 4112,), "bit31", "fq_resident.hip: fq_add_resident", "operand bytes",
       2 * ((1 << 30) + 4112), None, 2 * ((1 << 30) + 4112), 7 * ((1 << 30) + 4112)),
    _g("dequant_2_30", "fq_dequant_nhwc_to_nchw", (131, 200, 41003, 208), "bit31", "fq_resident.hip: fq_dequant_nhwc_to_nchw",
       "y bytes", 4 * prod(131, 200, 41003), None, 4 * prod(131, 200, 41003), prod(131, 41003, 208) + 4 * prod(131, 200, 41003)),
    _g("avgpool_global_i16", "fq_avgpool_global_nhwc", (1031, 2040, 511, 2048), "bit31", "fq_resident.hip: fq_avgpool_global_nhwc",
       "q bytes", 2 * prod(1031, 511, 2048), None, 2 * prod(1031, 511, 2048), 2 * prod(1031, 511, 2048)),
    _g("quantize_general_vec", "fq_quantize_i8_nhwc", (131, 200, 82004, 208), "bit31", "fq_conv_i8.hip: fq_quantize_i8_nhwc", "x elements",
       prod(131, 200, 82004), None, 4 * prod(131, 200, 82004), 4 * prod(131, 200, 82004) + prod(131, 82004, 208)),
    _g("quantize_general_odd", "fq_quantize_i8_nhwc", (131, 200, 82003, 208), "bit31", "fq_conv_i8.hip: fq_quantize_i8_nhwc", "x elements",
       prod(131, 200, 82003), None, 4 * prod(131, 200, 82003), 4 * prod(131, 200, 82003) + prod(131, 82003, 208)),
    _g("quantize_rows", "fq_quantize_i8_nhwc", (32779, 65521, 1, 65536), "bit31", "fq_conv_i8.hip: fq_quantize_i8_nhwc", "x elements",
       prod(32779, 65521), None, 4 * prod(32779, 65521), 4 * prod(32779, 65521) + prod(32779, 65536)),
    _g("quantize_smallc", "fq_quantize_i8_nhwc", (2731, 3, 262147, 16), "bit31", "fq_conv_i8.hip: fq_quantize_i8_nhwc", "x elements",
       prod(2731, 3, 262147), None, 4 * prod(2731, 3, 262147), 4 * prod(2731, 3, 262147) + prod(2731, 262147, 16)),
]

# walker program (scripts/) -> its arguments for the top row of the same name: the first and the last 4096 pixels of the launch,
# walked on the host before the row ran on a device (tests/test_size_guards_cpu.py runs them)
WALKER_ROWS = {
    "cat_top": ("concat_geom_check.cpp", ["window=4096", "maxsrc=2", "520,254,254/20,44/2,1"]),
    "catn_top": ("concat_geom_check.cpp", ["window=4096", "520,254,254/20,3,41/2,1,1"]),
    "avgi_top": ("avgpool_geom_check.cpp", ["window=65536", "4160,127,127,19,3,3,1,1,1,1"]),
    "dwf_top": ("dwconv_f32_geom_check.cpp", ["window=4096", "128,520,127,127,3,1,1"]),
    "gf_top": ("gconv_f32_geom_check.cpp", ["window=2048", "1109,5,4,12,127,127,3,1,1"]),
    "gci_top": ("gconv_geom_check.cpp", ["window=1024", "5,4,12,3,1,1,1040,127,127"]),
    "dwi_top": ("dwconv_geom_check.cpp", ["window=4096", "3,1,2080,127,127,19,1"]),
}

# top rows whose shape is a workload's, not a ragged one: ResNet-101 at 512 x 512 (golden G13) at the largest admitted batch
WORKLOAD_ROWS = {"stem_f32_r101_512_b255"}

# the entry points of the issue's list that have no GPU row yet, and why (their guards ARE in REFUSALS)
NOT_RUN = {
    "fq_conv2d_i8 at the top on the two halo kernels and the streaming 1x1 kernel": "the halo kernels take stride-1 3x3 layers with "
    "C % 128 == 0 only and no row of the issue's list reaches them (its 3x3 rows are stride 2 or C = 64); the streaming kernel is "
    "opt-in (FQ_CONV_STREAM=1) and a row names the kernel reached without a switch -- its own host check keeps it 256 KB of input "
    "and 2^30 output bytes away from 2^31",
}
