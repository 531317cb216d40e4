// fq_gconv_i8.hip -- grouped int8 convolution, 1 < groups < channels, on resident activations (include/fq.h:
// fq_gconv2d_i8_resident).  G = groups, Cgi = C / G, Cgo = K / G:
//
//   acc[n][k][p][q] = sum_{r,s} sum_{j < Cgi} w[k][j][r][s] * x[n][p*stride - pad + r][q*stride - pad + s][(k / Cgo) * Cgi + j]
//   q_out           = clamp(RightShift(acc, rs or rs_k[k]) + qbias[k]),   ReLU fused when relu != 0
//
// With 4 .. 64 input channels per group an int8 MFMA tile would be mostly zeros; four consecutive input channels of one pixel
// are one dword of NHWC, so v_dot4_i32_i8 sums them without any transpose:
//   * one lane owns 4 consecutive output channels (one output dword; one group, because Cgo % 4 == 0) and a strip of kGcTQ
//     output pixels of one row;
//   * per kernel row and 4-channel chunk it loads the (kGcTQ - 1) * stride + S input dwords its strip touches (zero outside
//     the image, never clamped onto the border), and per tap one 16-byte weight unit: dword i = the four input channels of the
//     chunk for output channel i.  16 dot4 per tap and chunk;
//   * a workgroup keeps ONE block of 64 / 32 / 16 output channels (the largest that divides Kpad) while it steps over the strips;
//     that block's weights (at most 64 x 9 x 64 B = 36 KB) are staged in LDS once, quads innermost, so the lanes of a wave read
//     consecutive units;
//   * neighbouring lanes are neighbouring channel quads of the same strip, so a wave stores whole contiguous pixel segments and,
//     for Cgi = 4, loads them too;
//   * the three tail constants per channel (fq_int_tail.h: tail_consts / conv_tail_k) stay in registers; at most 2048 workgroups.
// Output quads at or beyond K are padding: they load nothing and write zeros (tail constants 0, 0, 0).  Every index comes from
// fq_gconv_i8_geom.h, which scripts/gconv_geom_check.cpp compiles as host code and walks over the test shapes.
#include "fq_common.h"
#include "fq_int_tail.h"
#include "fq_gconv_i8_geom.h"

namespace fq {

constexpr int kVarGrouped = 15;        // fq_conv2d_i8_last_variant

struct GcParams {
    GcGeom g;
    int rs, half_rs;                   // per-tensor shift (the per-channel form reads rs_k)
    int ilo, ihi, slo, shi;            // RightShift range, Sp range (slo = 0 with the fused ReLU)
};

template <int R, int STRIDE, bool PCS>
__global__ __launch_bounds__(kGcBlock) void gconv_i8_kernel(const int8_t* __restrict__ x, const int8_t* __restrict__ w,
                                                           const float* __restrict__ qbias, const int32_t* __restrict__ rs_k,
                                                           int8_t* __restrict__ q, const GcParams p) {
    constexpr int S = R, TQ = kGcTQ;
    constexpr int NPIX = (TQ - 1) * STRIDE + S;           // input columns of a strip
    extern __shared__ uint4 gc_lds[];                     // g.units weight units
    const GcGeom& g = p.g;
    const int kb = gc_block_kb(g, blockIdx.x);
    for (unsigned i = threadIdx.x; i < g.units; i += kGcBlock)
        gc_lds[gc_stage_dst(g, i)] = reinterpret_cast<const uint4*>(w)[gc_stage_src(g, kb, i)];
    __syncthreads();

    const int kql = gc_lane_quad(g, (int)threadIdx.x), ls = gc_lane_strip(g, (int)threadIdx.x);
    const int kq = gc_quad(g, kb, kql);
    const bool valid = gc_quad_valid(g, kq);
    // the tail of each channel: rounding constant with the bias in it, merged clamp bounds, shift
    int tB[4], tlo[4], thi[4], trs[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int ch = 4 * kq + c;
        if (valid) {
            const int qb = (int)qbias[ch];                // integer valued by contract; the conversion saturates
            TailK k;
            if constexpr (PCS) { trs[c] = rs_k[ch]; k = tail_consts_rs(qb, p, trs[c]); }
            else { trs[c] = p.rs; k = tail_consts(qb, p); }
            tB[c] = k.B; tlo[c] = k.lo; thi[c] = k.hi;
        } else {
            tB[c] = 0; tlo[c] = 0; thi[c] = 0; trs[c] = 1;
        }
    }

    const unsigned step = gc_sb_step(g, gridDim.x);
    for (unsigned sb = gc_block_sb0(g, blockIdx.x); sb < g.sblocks; sb += step) {
        const unsigned strip = sb * (unsigned)g.SPW + (unsigned)ls;
        if (strip >= g.strips) continue;
        const GcStripPos sp = gc_strip_pos(g, strip);
        const int ih0 = sp.p * STRIDE - g.pad_h, iw0 = sp.q0 * STRIDE - g.pad_w;
        int acc[4][TQ];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < TQ; ++j) acc[c][j] = 0;

        if (valid) {
            for (int j4 = 0; j4 < g.CH; ++j4) {
                const int chan = gc_in_chan(g, kq, j4);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int ih = ih0 + r;
                    unsigned xv[NPIX];
#pragma unroll
                    for (int k = 0; k < NPIX; ++k) {
                        xv[k] = 0u;
                        if (gc_in_ok(g, ih, iw0 + k)) xv[k] = *reinterpret_cast<const unsigned*>(x + gc_in_off(g, sp.n, ih, iw0 + k, chan));
                    }
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const uint4 wv = gc_lds[gc_lds_unit(g, kql, r * S + s, j4)];
#pragma unroll
                        for (int j = 0; j < TQ; ++j) {
                            const int xi = (int)xv[j * STRIDE + s];
                            acc[0][j] = __builtin_amdgcn_sdot4(xi, (int)wv.x, acc[0][j], false);
                            acc[1][j] = __builtin_amdgcn_sdot4(xi, (int)wv.y, acc[1][j], false);
                            acc[2][j] = __builtin_amdgcn_sdot4(xi, (int)wv.z, acc[2][j], false);
                            acc[3][j] = __builtin_amdgcn_sdot4(xi, (int)wv.w, acc[3][j], false);
                        }
                    }
                }
            }
        }

#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            int v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = conv_tail_k(acc[c][j], tB[c], tlo[c], thi[c], trs[c]);
            if (gc_out_ok(g, sp.q0 + j))
                *reinterpret_cast<unsigned*>(q + gc_out_off(g, sp.n, sp.p, sp.q0 + j, kq)) = pack4(v[0], v[1], v[2], v[3]);
        }
    }
}

static bool gc_supported(int C, int K, int groups, int R, int S, int stride_h, int stride_w, int dil_h, int dil_w, int rs_min,
                         int rs_max) {
    if (groups < 2 || C < 1 || K < 1 || C % groups || K % groups) return false;
    const int cgi = C / groups, cgo = K / groups;
    return cgi % 4 == 0 && cgo % 4 == 0 && cgi >= 4 && cgi <= 64 && cgo >= 4 && cgo <= 64 && R == S && (R == 1 || R == 3) &&
           stride_h == stride_w && (stride_h == 1 || stride_h == 2) && dil_h == 1 && dil_w == 1 && rs_min >= 1 &&
           rs_min <= rs_max && rs_max <= 16;
}

template <bool PCS>
static void gc_launch(int R, int stride, unsigned blocks, size_t lds, hipStream_t st, const int8_t* x, const int8_t* w,
                      const float* qbias, const int32_t* rs_k, int8_t* q, const GcParams& p) {
    if (R == 1 && stride == 1) gconv_i8_kernel<1, 1, PCS><<<blocks, kGcBlock, lds, st>>>(x, w, qbias, rs_k, q, p);
    else if (R == 1) gconv_i8_kernel<1, 2, PCS><<<blocks, kGcBlock, lds, st>>>(x, w, qbias, rs_k, q, p);
    else if (stride == 1) gconv_i8_kernel<3, 1, PCS><<<blocks, kGcBlock, lds, st>>>(x, w, qbias, rs_k, q, p);
    else gconv_i8_kernel<3, 2, PCS><<<blocks, kGcBlock, lds, st>>>(x, w, qbias, rs_k, q, p);
}

static int gconv_dispatch(const int8_t* x_nhwc, const int8_t* w_pack, const float* qbias, const int32_t* rs_k, int rs_min,
                          int rs_max, int8_t* q_nhwc, int Cpad, int Kpad, SpRange sp, int N, int H, int W, int C, int K, int groups,
                          int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int ob,
                          fq_stream_t stream) {
    if (!sp_range_valid(sp)) return FQ_ERR_INVALID_ARG;   // (the Sp range: [-128, 127], [0, 127] with a ReLU, or an _act caller's)
    if (rs_min < -120 || rs_max > 120 || rs_min > rs_max || ob < -120 || ob > 120) return FQ_ERR_INVALID_ARG;
    if (rs_k && (reinterpret_cast<uintptr_t>(rs_k) & 15u)) return FQ_ERR_INVALID_ARG;
    if (N < 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0 || groups <= 0 || R <= 0 || S <= 0 || stride_h <= 0 || stride_w <= 0 ||
        pad_h < 0 || pad_w < 0 || dil_h <= 0 || dil_w <= 0)
        return FQ_ERR_INVALID_ARG;
    if (C % groups || K % groups) return FQ_ERR_INVALID_ARG;
    if (Cpad != (C + 15) / 16 * 16 || Kpad != (K + 15) / 16 * 16) return FQ_ERR_INVALID_ARG;
    if (!gc_supported(C, K, groups, R, S, stride_h, stride_w, dil_h, dil_w, rs_min, rs_max) || pad_h >= R || pad_w >= S)
        return FQ_ERR_UNSUPPORTED;
    if (H + 2 * pad_h < R || W + 2 * pad_w < S) return FQ_ERR_INVALID_ARG;
    g_last_conv_variant = kVarNone;
    if (N == 0) return FQ_OK;
    if (!x_nhwc || !w_pack || !qbias || !q_nhwc) return FQ_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(x_nhwc) | reinterpret_cast<uintptr_t>(w_pack) | reinterpret_cast<uintptr_t>(q_nhwc)) & 15u)
        return FQ_ERR_INVALID_ARG;
    const int P = (H + 2 * pad_h - R) / stride_h + 1, Q = (W + 2 * pad_w - S) / stride_w + 1;
    // 32-bit element offsets into both activations, 32-bit strip indices
    if ((long)N * H * W * Cpad >= 0x7fffffffL || (long)N * P * Q * Kpad >= 0x3fffffffL) return FQ_ERR_UNSUPPORTED;
    GcParams p;
    if (!gc_setup(p.g, N, H, W, C, K, groups, R, stride_h, pad_h, pad_w)) return FQ_ERR_UNSUPPORTED;
    // accumulator bound of the integer tail (fq_int_tail.h): 9 * 64 * 128 * 128 < 2^24, bias term below 2^(9 + 16)
    p.rs = rs_min; p.half_rs = 1 << (rs_min - 1);
    // (any Sp range inside [-128, 127] keeps tail_consts' bias clamp inside [-255, 255])
    p.ilo = -128; p.ihi = 127; p.slo = sp.lo; p.shi = sp.hi;
    hipStream_t st = as_stream(stream);
    const unsigned blocks = gc_blocks(p.g);
    const size_t lds = (size_t)p.g.units * kGcUnit;
    if (rs_k) gc_launch<true>(R, stride_h, blocks, lds, st, x_nhwc, w_pack, qbias, rs_k, q_nhwc, p);
    else gc_launch<false>(R, stride_h, blocks, lds, st, x_nhwc, w_pack, qbias, nullptr, q_nhwc, p);
    note_conv_variant(kVarGrouped, 0);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace fq

using namespace fq;

extern "C" int fq_gconv2d_i8_supported(int C, int K, int groups, int R, int S, int stride_h, int stride_w, int dil_h, int dil_w,
                                       int rs_min, int rs_max) {
    return gc_supported(C, K, groups, R, S, stride_h, stride_w, dil_h, dil_w, rs_min, rs_max) ? 1 : 0;
}

extern "C" int fq_gconv2d_i8_resident(const int8_t* x_nhwc, const int8_t* w_pack, const float* qbias, int8_t* q_nhwc, int Cpad,
                                      int Kpad, int relu, int N, int H, int W, int C, int K, int groups, int R, int S,
                                      int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int rs, int ob,
                                      fq_stream_t stream) {
    return gconv_dispatch(x_nhwc, w_pack, qbias, nullptr, rs, rs, q_nhwc, Cpad, Kpad, sp_range_relu(relu), N, H, W, C, K, groups, R, S, stride_h,
                          stride_w, pad_h, pad_w, dil_h, dil_w, ob, stream);
}

extern "C" int fq_gconv2d_i8_resident_pcs(const int8_t* x_nhwc, const int8_t* w_pack, const float* qbias, const int32_t* rs_k,
                                          int rs_min, int rs_max, int8_t* q_nhwc, int Cpad, int Kpad, int relu, int N, int H,
                                          int W, int C, int K, int groups, int R, int S, int stride_h, int stride_w, int pad_h,
                                          int pad_w, int dil_h, int dil_w, int ob, fq_stream_t stream) {
    if (!rs_k && N > 0) return FQ_ERR_INVALID_ARG;
    return gconv_dispatch(x_nhwc, w_pack, qbias, rs_k, rs_min, rs_max, q_nhwc, Cpad, Kpad, sp_range_relu(relu), N, H, W, C, K, groups, R, S,
                          stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, ob, stream);
}

extern "C" int fq_gconv2d_i8_resident_act(const int8_t* x_nhwc, const int8_t* w_pack, const float* qbias, int8_t* q_nhwc, int Cpad,
                                          int Kpad, int act_lo, int act_hi, int N, int H, int W, int C, int K, int groups, int R,
                                          int S, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int rs,
                                          int ob, fq_stream_t stream) {
    return gconv_dispatch(x_nhwc, w_pack, qbias, nullptr, rs, rs, q_nhwc, Cpad, Kpad, SpRange{act_lo, act_hi}, N, H, W, C, K, groups,
                          R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, ob, stream);
}

extern "C" int fq_gconv2d_i8_resident_pcs_act(const int8_t* x_nhwc, const int8_t* w_pack, const float* qbias, const int32_t* rs_k,
                                              int rs_min, int rs_max, int8_t* q_nhwc, int Cpad, int Kpad, int act_lo, int act_hi,
                                              int N, int H, int W, int C, int K, int groups, int R, int S, int stride_h, int stride_w,
                                              int pad_h, int pad_w, int dil_h, int dil_w, int ob, fq_stream_t stream) {
    if (!rs_k && N > 0) return FQ_ERR_INVALID_ARG;
    return gconv_dispatch(x_nhwc, w_pack, qbias, rs_k, rs_min, rs_max, q_nhwc, Cpad, Kpad, SpRange{act_lo, act_hi}, N, H, W, C, K,
                          groups, R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, ob, stream);
}
