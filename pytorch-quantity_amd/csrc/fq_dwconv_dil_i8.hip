// fq_dwconv_dil_i8.hip -- atrous (dilated) depthwise int8 convolution on resident activations
// (include/fq.h: fq_dwconv2d_dil_i8_resident): the depthwise layers of a backbone that trades stride for dilation and the
// 3x3 branches of an atrous-separable ASPP.
//
//   acc[n][c][p][q] = sum_{r,s} w[c][r][s] * x[n][p - pad_h + r*d][q - pad_w + s*d][c]            (int32, exact)
//   q_out           = clamp(RightShift(acc, rs or rs_k[c]) + qbias[c]),   ReLU fused when relu != 0
//
// The dense kernel (fq_dwconv_i8.hip) lives on v_dot4_i32_i8 over the taps of one kernel row in CONSECUTIVE pixels; with
// dilation the taps are d pixels apart.  They are consecutive again on the lattice of step d through the output pixel's phase
// (fq_dwconv_dil_i8_geom.h): a stride-1 convolution with dilation d is d x d independent dense stride-1 convolutions, one per
// (p mod d, q mod d).  So:
//   * one lane owns 4 consecutive channels (one dword of an NHWC pixel) and a tile of TP x 4 outputs of ONE phase: rows
//     fh + d*(pp0 + t), columns fw + d*(qq0 + j);
//   * per lattice row it loads the 3 + S dwords its four output columns touch, at a pixel step of d (zero outside the image),
//     transposes every 4 pixels x 4 channels and slides the window with v_alignbyte_b32, and accumulates with sdot4 (a 5-tap row:
//     a second sdot4 for the fifth pixel) -- the register and ALU work of the dense kernel at stride 1, word for word
//     (fq_dwconv_i8_lane.h holds what the two share);
//   * a transposed lattice row serves every output row of the tile that reads it;
//   * weights and the three tail constants per channel stay in registers while the lane strides over its tiles: at most 2048
//     workgroups of 256; the lane decodes its first tile and its stride once and then advances the (image, band, row phase,
//     block, column phase) digits with carries (dwd_advance), so the runtime d costs no division inside the tile loop;
//   * tiles are numbered with the column phase fastest: neighbouring tiles are neighbouring pixels, 4 lanes cover 16 contiguous
//     bytes, and for C4 < 64 a wave's loads and stores cover contiguous bytes; the d phases of a line hit the same cache lines
//     close in time, so HBM sees every input line once per kernel row, as in the dense kernel.
// What the split costs: a phase sub-plane has ceil((Q - fw) / d) columns, so where Q < 4d most of a tile's columns are
// predicated off (DESIGN: the utilisation arithmetic).  Loads are predicated on the image bounds, stores on the output
// bounds; every offset is below N*H*W*Cpad / N*P*Q*Cpad (scripts/dwconv_dil_geom_check.cpp walks the test shapes on the host).
// Channels [C, Cpad) are written as zeros whatever the input's padding channels hold: their tail constants are (0, 0, 0).
#include "fq_common.h"
#include "fq_int_tail.h"
#include "fq_dwconv_dil_i8_geom.h"
#include "fq_dwconv_i8_lane.h"

namespace fq {

constexpr int kVarDepthwiseDilated = 17;   // fq_conv2d_i8_last_variant

struct DwDilParams {
    DwDilGeom a;
    int C;
    int rs, half_rs;                   // per-tensor shift (the per-channel form reads rs_k)
    int ilo, ihi, slo, shi;            // RightShift range, Sp range (slo = 0 with the fused ReLU)
};

template <int R, bool PCS>
__global__ __launch_bounds__(kDwBlock) void dwconv_dil_i8_kernel(const int8_t* __restrict__ x, const int8_t* __restrict__ w,
                                                                const float* __restrict__ qbias, const int32_t* __restrict__ rs_k,
                                                                int8_t* __restrict__ q, const DwDilParams p) {
    constexpr int S = R, TP = DwTile<R>::TP, TQ = kDwTQ;
    constexpr int NROWS = TP - 1 + R;                     // lattice rows of a tile
    constexpr int NPIX = TQ - 1 + S;                      // lattice columns of a tile
    constexpr int NG = (NPIX + 3) / 4;                    // transposed groups of 4 lattice pixels
    const DwDilGeom& a = p.a;
    const DwGeom& g = a.g;
    const unsigned gid = blockIdx.x * kDwBlock + threadIdx.x;
    const unsigned sp_stride = (gridDim.x * kDwBlock) / (unsigned)g.C4;
    const int c4 = (int)(gid % (unsigned)g.C4);
    unsigned tile = gid / (unsigned)g.C4;
    if (tile >= sp_stride) return;

    // this lane's weights: wr[r][c] = taps 0..3 of row r (byte s), w4[r][c] = tap 4 in byte 0 (5x5)
    unsigned wr[R][4], w4[S == 5 ? R : 1][4];
    dw_lane_weights<R>(w, g.Cpad, c4, wr, w4);
    // the tail of each channel: rounding constant with the bias in it, merged clamp bounds, shift
    int tB[4], tlo[4], thi[4], trs[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int ch = 4 * c4 + c;
        if (ch < p.C) {
            const int qb = (int)qbias[ch];                // integer valued by contract; the conversion saturates
            TailK k;
            if constexpr (PCS) { trs[c] = rs_k[ch]; k = tail_consts_rs(qb, p, trs[c]); }
            else { trs[c] = p.rs; k = tail_consts(qb, p); }
            tB[c] = k.B; tlo[c] = k.lo; thi[c] = k.hi;
        } else {
            tB[c] = 0; tlo[c] = 0; thi[c] = 0; trs[c] = 1;
        }
    }

    const int d = a.d;
    DwDilPos pos = dwd_decode(a, tile);                   // the only divisions: the first tile and the stride
    const DwDilPos step = dwd_decode(a, sp_stride);
    for (; tile < g.tiles; tile += sp_stride, dwd_advance(a, pos, step)) {
        const DwDilTile tl = dwd_tile<TP>(a, pos);
        if (!dw_out_ok(g, tl.p0, tl.q0)) continue;        // a band or block beyond this (shorter) phase's sub-plane
        int acc[TP][4][TQ];
#pragma unroll
        for (int t = 0; t < TP; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int j = 0; j < TQ; ++j) acc[t][c][j] = 0;

#pragma unroll
        for (int i = 0; i < NROWS; ++i) {
            const int ih = tl.ih0 + i * d;
            unsigned T[NG][4];
#pragma unroll
            for (int gg = 0; gg < NG; ++gg) {
                unsigned dd[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int pix = 4 * gg + k, iw = tl.iw0 + pix * d;
                    dd[k] = 0u;
                    if (pix < NPIX && dw_in_ok(g, ih, iw)) dd[k] = *reinterpret_cast<const unsigned*>(x + dw_in_off(g, pos.n, ih, iw, c4));
                }
                transpose4(dd, T[gg]);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int j = 0; j < TQ; ++j) {                // window j = lattice pixels j .. j + 3 (compile time after unrolling)
                    const int ga = j / 4;
                    const unsigned win = dw_window(T[ga][c], T[ga + (ga + 1 < NG ? 1 : 0)][c], j % 4);
                    unsigned fifth = 0u;
                    if constexpr (S == 5) fifth = dw_fifth(T[(j + 4) / 4][c], (j + 4) % 4);
#pragma unroll
                    for (int t = 0; t < TP; ++t) {
                        const int r = i - t;                  // the kernel row through which lattice row i reaches output row t
                        if (r >= 0 && r < R) {
                            acc[t][c][j] = __builtin_amdgcn_sdot4((int)win, (int)wr[r][c], acc[t][c][j], false);
                            if constexpr (S == 5) acc[t][c][j] = __builtin_amdgcn_sdot4((int)fifth, (int)w4[r][c], acc[t][c][j], false);
                        }
                    }
                }
            }
        }

#pragma unroll
        for (int t = 0; t < TP; ++t) {
#pragma unroll
            for (int j = 0; j < TQ; ++j) {
                int v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = conv_tail_k(acc[t][c][j], tB[c], tlo[c], thi[c], trs[c]);
                const int pp = tl.p0 + t * d, qq = tl.q0 + j * d;
                if (dw_out_ok(g, pp, qq))
                    *reinterpret_cast<unsigned*>(q + dw_out_off(g, pos.n, pp, qq, c4)) = pack4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

static bool dwd_supported(int C, int R, int S, int stride_h, int stride_w, int dil_h, int dil_w, int rs_min, int rs_max) {
    return C >= 1 && R == S && (R == 3 || R == 5) && stride_h == 1 && stride_w == 1 && dil_h == dil_w && dil_h >= kDwDilMin &&
           dil_h <= kDwDilMax && rs_min >= 1 && rs_min <= rs_max && rs_max <= 16;
}

template <bool PCS>
static void dwd_launch(int R, unsigned blocks, hipStream_t st, const int8_t* x, const int8_t* w, const float* qbias,
                       const int32_t* rs_k, int8_t* q, const DwDilParams& p) {
    if (R == 3) dwconv_dil_i8_kernel<3, PCS><<<blocks, kDwBlock, 0, st>>>(x, w, qbias, rs_k, q, p);
    else dwconv_dil_i8_kernel<5, PCS><<<blocks, kDwBlock, 0, st>>>(x, w, qbias, rs_k, q, p);
}

static int dwconv_dil_dispatch(const int8_t* x_nhwc, const int8_t* w_rsc, const float* qbias, const int32_t* rs_k, int rs_min,
                               int rs_max, int8_t* q_nhwc, int Cpad, SpRange sp, int N, int H, int W, int C, int R, int S,
                               int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int ob, fq_stream_t stream) {
    if (!sp_range_valid(sp)) return FQ_ERR_INVALID_ARG;   // (the Sp range: [-128, 127], [0, 127] with a ReLU, or an _act caller's)
    if (rs_min < -120 || rs_max > 120 || rs_min > rs_max || ob < -120 || ob > 120) return FQ_ERR_INVALID_ARG;
    if (rs_k && (reinterpret_cast<uintptr_t>(rs_k) & 15u)) return FQ_ERR_INVALID_ARG;
    if (N < 0 || H <= 0 || W <= 0 || C <= 0 || R <= 0 || S <= 0 || stride_h <= 0 || stride_w <= 0 || pad_h < 0 || pad_w < 0 ||
        dil_h <= 0 || dil_w <= 0)
        return FQ_ERR_INVALID_ARG;
    if (Cpad % 16) return FQ_ERR_UNSUPPORTED;             // as fq_conv2d_i8_resident: pad channels to 16
    if (Cpad < C) return FQ_ERR_INVALID_ARG;
    if (!dwd_supported(C, R, S, stride_h, stride_w, dil_h, dil_w, rs_min, rs_max)) return FQ_ERR_UNSUPPORTED;
    const int d = dil_h, span = d * (R - 1);              // (the window covers span + 1 pixels)
    if (pad_h > span || pad_w > span) return FQ_ERR_UNSUPPORTED;
    if ((long)H + 2 * pad_h <= span || (long)W + 2 * pad_w <= span) return FQ_ERR_INVALID_ARG;
    const int P = H + 2 * pad_h - span, Q = W + 2 * pad_w - span;
    g_last_conv_variant = kVarNone;
    if (N == 0) return FQ_OK;
    if (!x_nhwc || !w_rsc || !qbias || !q_nhwc) return FQ_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(x_nhwc) | reinterpret_cast<uintptr_t>(w_rsc) | reinterpret_cast<uintptr_t>(q_nhwc)) & 15u)
        return FQ_ERR_INVALID_ARG;
    // 32-bit element offsets into both activations; the channel groups of one pixel fit the launch
    if ((long)N * H * W * Cpad >= 0x7fffffffL || (long)N * P * Q * Cpad >= 0x3fffffffL || Cpad > 65536) return FQ_ERR_UNSUPPORTED;
    DwDilParams p;
    if (!dwd_make(p.a, R == 3 ? DwTile<3>::TP : DwTile<5>::TP, N, H, W, Cpad, R, d, pad_h, pad_w)) return FQ_ERR_UNSUPPORTED;
    p.C = C;
    // accumulator bound of the integer tail (fq_int_tail.h): 25 * 128 * 128 < 2^19, bias term below 2^(9 + 16)
    p.rs = rs_min; p.half_rs = 1 << (rs_min - 1);
    // (any Sp range inside [-128, 127] keeps tail_consts' bias clamp inside [-255, 255])
    p.ilo = -128; p.ihi = 127; p.slo = sp.lo; p.shi = sp.hi;
    const unsigned blocks = dwd_blocks(p.a);
    hipStream_t st = as_stream(stream);
    if (rs_k) dwd_launch<true>(R, blocks, st, x_nhwc, w_rsc, qbias, rs_k, q_nhwc, p);
    else dwd_launch<false>(R, blocks, st, x_nhwc, w_rsc, qbias, nullptr, q_nhwc, p);
    note_conv_variant(kVarDepthwiseDilated, 0);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace fq

using namespace fq;

extern "C" int fq_dwconv2d_dil_i8_supported(int C, int R, int S, int stride_h, int stride_w, int dil_h, int dil_w, int rs_min,
                                            int rs_max) {
    return dwd_supported(C, R, S, stride_h, stride_w, dil_h, dil_w, rs_min, rs_max) ? 1 : 0;
}

extern "C" int fq_dwconv2d_dil_i8_resident(const int8_t* x_nhwc, const int8_t* w_rsc, const float* qbias, int8_t* q_nhwc, int Cpad,
                                           int relu, int N, int H, int W, int C, int R, int S, int stride_h, int stride_w, int pad_h,
                                           int pad_w, int dil_h, int dil_w, int rs, int ob, fq_stream_t stream) {
    return dwconv_dil_dispatch(x_nhwc, w_rsc, qbias, nullptr, rs, rs, q_nhwc, Cpad, sp_range_relu(relu), N, H, W, C, R, S, stride_h,
                               stride_w, pad_h, pad_w, dil_h, dil_w, ob, stream);
}

extern "C" int fq_dwconv2d_dil_i8_resident_pcs(const int8_t* x_nhwc, const int8_t* w_rsc, const float* qbias, const int32_t* rs_k,
                                               int rs_min, int rs_max, int8_t* q_nhwc, int Cpad, int relu, int N, int H, int W, int C,
                                               int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                               int ob, fq_stream_t stream) {
    if (!rs_k && N > 0) return FQ_ERR_INVALID_ARG;
    return dwconv_dil_dispatch(x_nhwc, w_rsc, qbias, rs_k, rs_min, rs_max, q_nhwc, Cpad, sp_range_relu(relu), N, H, W, C, R, S,
                               stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, ob, stream);
}

extern "C" int fq_dwconv2d_dil_i8_resident_act(const int8_t* x_nhwc, const int8_t* w_rsc, const float* qbias, int8_t* q_nhwc,
                                               int Cpad, int act_lo, int act_hi, int N, int H, int W, int C, int R, int S,
                                               int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int rs, int ob,
                                               fq_stream_t stream) {
    return dwconv_dil_dispatch(x_nhwc, w_rsc, qbias, nullptr, rs, rs, q_nhwc, Cpad, SpRange{act_lo, act_hi}, N, H, W, C, R, S,
                               stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, ob, stream);
}

extern "C" int fq_dwconv2d_dil_i8_resident_pcs_act(const int8_t* x_nhwc, const int8_t* w_rsc, const float* qbias,
                                                   const int32_t* rs_k, int rs_min, int rs_max, int8_t* q_nhwc, int Cpad, int act_lo,
                                                   int act_hi, int N, int H, int W, int C, int R, int S, int stride_h, int stride_w,
                                                   int pad_h, int pad_w, int dil_h, int dil_w, int ob, fq_stream_t stream) {
    if (!rs_k && N > 0) return FQ_ERR_INVALID_ARG;
    return dwconv_dil_dispatch(x_nhwc, w_rsc, qbias, rs_k, rs_min, rs_max, q_nhwc, Cpad, SpRange{act_lo, act_hi}, N, H, W, C, R, S,
                               stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, ob, stream);
}
