// fq_deconv_i8.hip -- transposed convolution (nn.ConvTranspose2d, groups 1, dilation 1) on resident int8 activations
// (include/fq.h: fq_deconv2d_i8_resident).
//
//   P = (H-1) sh - 2 ph + R + oph,  Q = (W-1) sw - 2 pw + S + opw
//   acc[n][oh][ow][k] = sum x[n][ih][iw][c] w[c][k][r][s]   over c < C and the taps with oh + ph - r = ih sh, ow + pw - s = iw sw
//   q = clamp(RightShift(acc, rs) + qbias[k])                (fq_int_tail.h, the dense kernel's tail; ReLU / Sp range fused)
//
// Sub-pixel phases on the int8 matrix cores.  The output pixels with the same ((oh + ph) mod sh, (ow + pw) mod sw) form a dense
// stride-1 correlation over x with the taps r = a (mod sh), s = b (mod sw) only (fq_deconv_i8_geom.h), so no product with a
// stuffed zero is ever issued: a zero-stuffed implicit GEMM would spend 1 - 1 / (sh sw) of its MFMAs on them.
//   * the weights are packed per phase as [phase][k][tap][c16]: a phase's reduction axis is a run of 16-byte chunks (16 input
//     channels of one tap), and one chunk is exactly a lane's operand of v_mfma_i32_32x32x32_i8 -- half-wave 0 takes the even
//     chunks, half-wave 1 the odd ones, for both operands alike;
//   * weights are operand A, activations operand B: lane l of either half-wave owns pixel l of the wave's 32, and register e of
//     the accumulator is channel (e & 3) + 8 (e >> 2) + 4 half, so a lane holds runs of four consecutive channels of ONE pixel;
//   * both operands come straight from L2 into the MFMA's registers by buffer loads, one aligned 16-byte load per lane, operand
//     and step; a tap outside the image, a masked pixel, a chunk past the (odd) end of the axis and a weight row past Kpad get an
//     offset beyond num_records and read zeros (fq_conv_i8_common.h): no select, no zero page;
//   * a workgroup of four waves takes 128 pixels x KW channels (KW = 32, or 64 where Kpad > 32: two accumulators per activation
//     fragment) of one phase; at most 2048 workgroups stride over the items, the (phase, block, tile) and (n, row, column)
//     digits advanced by additions and carries (dc_walk_step);
//   * the tail constants of the item's channels are staged in LDS once per item (tail_consts); the epilogue packs four channels
//     per register run (pack4), exchanges two dwords with the partner lane of the other half-wave (the same pixel, channels
//     +4) and stores 16 aligned bytes: 16 consecutive channels of one output pixel per lane.
// A phase without a tap (kernel 2, stride 4) runs no MFMA and stores tail(0, bias).  Channels [K, Kpad) carry zero weights and the
// constants (0, 0, 0): they are written as zeros.  The input's padding channels meet zero weights.
#include "fq_common.h"
#include "fq_int_tail.h"
#include "fq_conv_i8_common.h"
#include "fq_deconv_i8_geom.h"

namespace fq {

static_assert(kDcOk == FQ_OK && kDcInvalid == FQ_ERR_INVALID_ARG && kDcUnsupported == FQ_ERR_UNSUPPORTED, "the guard speaks fq.h's codes");
static_assert(kDcOutOfRange == kOutOfRange, "one out-of-range offset");

constexpr int kVarDeconv = 16;         // fq_conv2d_i8_last_variant
constexpr int kDcUnroll = 4;           // K-steps of operand loads in flight per wave

struct DcParams {
    DcGeom g;
    int rs, half_rs;
    int ilo, ihi, slo, shi;            // RightShift range, Sp range (slo = 0 with the fused ReLU)
};

template <int KT>
__global__ __launch_bounds__(kDcBlock) void deconv_i8_kernel(const int8_t* __restrict__ x, const int8_t* __restrict__ w,
                                                            const float* __restrict__ qbias, int8_t* __restrict__ q,
                                                            const DcParams p) {
    __shared__ __attribute__((aligned(16))) int sB[32 * KT], sLo[32 * KT], sHi[32 * KT];
    const DcGeom& g = p.g;
    const int tid = (int)threadIdx.x, lane = tid & 63, l32 = lane & 31, half = lane >> 5, wave = tid >> 6;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(x), 0, g.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(w), 0, g.w_bytes, 0x00020000);
    unsigned item = blockIdx.x;
    if (item >= g.items) return;
    DcWalk s = dc_walk_begin(g, item, (unsigned)(wave * 32 + l32));
    for (; item < g.items; item += g.blocks) {
        const DcPhase ph = dc_phase(g, s.f);
        const int k0 = (int)s.kb * g.KW;
        __syncthreads();                                      // the item before has read its constants
        if (tid < 32 * KT) {
            const int k = k0 + tid;
            TailK t{0, 0, 0};
            if (k < g.K) t = tail_consts((int)qbias[k], p);   // integer valued by contract; the conversion saturates
            sB[tid] = t.B; sLo[tid] = t.lo; sHi[tid] = t.hi;
        }
        const bool ok = dc_pix_ok(g, ph, s);
        v16i acc[KT];
#pragma unroll
        for (int a = 0; a < KT; ++a)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][e] = 0;
        DcChunk c = dc_chunk_begin();
        if (half) dc_chunk_next(g, ph, c);
        const int steps = (ph.chunks + 1) / 2;
        for (int st = 0; st < steps; st += kDcUnroll) {
            v4i fa[kDcUnroll][KT], fb[kDcUnroll];
#pragma unroll
            for (int u = 0; u < kDcUnroll; ++u) {
                if (st + u < steps) {
                    fb[u] = load_act(xr, dc_x_off(g, ph, s, ok, c));
#pragma unroll
                    for (int a = 0; a < KT; ++a) fa[u][a] = load_act(wr, dc_w_off(g, ph, k0 + 32 * a + l32, c.ch));
                    dc_chunk_next(g, ph, c);
                    dc_chunk_next(g, ph, c);
                }
            }
#pragma unroll
            for (int u = 0; u < kDcUnroll; ++u) {
                if (st + u < steps) {
#pragma unroll
                    for (int a = 0; a < KT; ++a) acc[a] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[u][a], fb[u], acc[a], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                      // the constants are staged
#pragma unroll
        for (int a = 0; a < KT; ++a) {
            unsigned d[4];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int kl = 32 * a + 8 * gq + 4 * half;    // dc_acc_channel(4 gq, half) of accumulator a
                const v4i B = *reinterpret_cast<const v4i*>(sB + kl), lo = *reinterpret_cast<const v4i*>(sLo + kl),
                          hi = *reinterpret_cast<const v4i*>(sHi + kl);
                int v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = conv_tail_k(acc[a][4 * gq + e], B[e], lo[e], hi[e], p.rs);
                d[gq] = pack4(v[0], v[1], v[2], v[3]);
            }
            // the partner lane of the other half-wave holds the same pixel's channels + 4: half 0 gathers channels 0 .. 15 of
            // the 32, half 1 channels 16 .. 31
            const unsigned ra = (unsigned)__shfl_xor((int)(half ? d[0] : d[2]), 32);
            const unsigned rb = (unsigned)__shfl_xor((int)(half ? d[1] : d[3]), 32);
            v4u out;
            if (half) { out.x = ra; out.y = d[2]; out.z = rb; out.w = d[3]; }
            else { out.x = d[0]; out.y = ra; out.z = d[1]; out.w = rb; }
            const int kc = k0 + 32 * a + 16 * half;
            if (ok && kc < g.Kpad) *reinterpret_cast<v4u*>(q + dc_q_off(g, ph, s, kc)) = out;
        }
        dc_walk_step(g, s);
    }
}

static int deconv_dispatch(const int8_t* x, const int8_t* w, const float* qbias, int8_t* q, int Cpad, int Kpad, SpRange sp, int N, int H,
                           int W, int C, int K, int R, int S, int sh, int sw, int ph, int pw, int oph, int opw, int rs, int ob,
                           fq_stream_t stream) {
    int launch = 0;
    const int rc = dc_guard(reinterpret_cast<uintptr_t>(x), reinterpret_cast<uintptr_t>(w), reinterpret_cast<uintptr_t>(qbias),
                            reinterpret_cast<uintptr_t>(q), Cpad, Kpad, sp.lo, sp.hi, N, H, W, C, K, R, S, sh, sw, ph, pw, oph, opw, rs, ob,
                            &launch);
    if (rc != FQ_OK) return rc;
    g_last_conv_variant = kVarNone;
    if (!launch) return FQ_OK;
    DcParams p;
    p.g = dc_geom(N, H, W, C, K, R, S, sh, sw, ph, pw, oph, opw);
    p.rs = rs; p.half_rs = 1 << (rs - 1);
    // (any Sp range inside [-128, 127] keeps tail_consts' bias clamp inside [-255, 255], the bound dc_supported is made with)
    p.ilo = -128; p.ihi = 127; p.slo = sp.lo; p.shi = sp.hi;
    hipStream_t st = as_stream(stream);
    if (p.g.KW == 64) deconv_i8_kernel<2><<<p.g.blocks, kDcBlock, 0, st>>>(x, w, qbias, q, p);
    else deconv_i8_kernel<1><<<p.g.blocks, kDcBlock, 0, st>>>(x, w, qbias, q, p);
    note_conv_variant(kVarDeconv, 0);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace fq

using namespace fq;

extern "C" int fq_deconv2d_i8_supported(int C, int K, int groups, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w,
                                        int outpad_h, int outpad_w, int dil_h, int dil_w, int rs_min, int rs_max) {
    return dc_supported(C, K, groups, R, S, stride_h, stride_w, pad_h, pad_w, outpad_h, outpad_w, dil_h, dil_w, rs_min, rs_max) ? 1 : 0;
}

extern "C" size_t fq_deconv2d_i8_packed_bytes(int C, int K, int R, int S) {
    return (C < 1 || K < 1 || R < 1 || S < 1) ? 0 : dc_packed_bytes(C, K, R, S);
}

extern "C" int fq_deconv2d_i8_resident(const int8_t* x_nhwc, const int8_t* w_pack, const float* qbias, int8_t* q_nhwc, int Cpad, int Kpad,
                                       int relu, int N, int H, int W, int C, int K, int R, int S, int stride_h, int stride_w, int pad_h,
                                       int pad_w, int outpad_h, int outpad_w, int rs, int ob, fq_stream_t stream) {
    return deconv_dispatch(x_nhwc, w_pack, qbias, q_nhwc, Cpad, Kpad, sp_range_relu(relu), N, H, W, C, K, R, S, stride_h, stride_w, pad_h,
                           pad_w, outpad_h, outpad_w, rs, ob, stream);
}

extern "C" int fq_deconv2d_i8_resident_act(const int8_t* x_nhwc, const int8_t* w_pack, const float* qbias, int8_t* q_nhwc, int Cpad,
                                           int Kpad, int act_lo, int act_hi, int N, int H, int W, int C, int K, int R, int S,
                                           int stride_h, int stride_w, int pad_h, int pad_w, int outpad_h, int outpad_w, int rs, int ob,
                                           fq_stream_t stream) {
    return deconv_dispatch(x_nhwc, w_pack, qbias, q_nhwc, Cpad, Kpad, SpRange{act_lo, act_hi}, N, H, W, C, K, R, S, stride_h, stride_w,
                           pad_h, pad_w, outpad_h, outpad_w, rs, ob, stream);
}
