// fq_dwconv_i8.hip -- depthwise int8 convolution on resident activations (include/fq.h: fq_dwconv2d_i8_resident).
//
//   acc[n][c][p][q] = sum_{r,s} w[c][r][s] * x[n][p*stride - pad + r][q*stride - pad + s][c]      (int32, exact)
//   q_out           = clamp(RightShift(acc, rs or rs_k[c]) + qbias[c]),   ReLU fused when relu != 0
//
// No sum over channels, so no matrix core: the work is R*S multiply-adds per output byte on the vector pipe, next to
// 2 bytes of HBM traffic.  One multiply-add per instruction with a byte unpack in front does not keep up with HBM;
// v_dot4_i32_i8 over the taps of one kernel row does:
//   * one lane owns 4 consecutive channels (one dword of an NHWC pixel) and a tile of TP x 4 output pixels;
//   * per input row it loads the 3*stride + S pixels its four output columns touch (a dword each, zero outside the image),
//     transposes every 4 pixels x 4 channels into 4 channels x 4 pixels (8 v_perm_b32) and slides the window with
//     v_alignbyte_b32: window j of channel c = pixels j*stride .. j*stride + 3;
//   * acc += dot4(window, (w[c][r][0], w[c][r][1], w[c][r][2], w[c][r][3] or 0)); a 5-tap row adds the fifth pixel with a
//     second dot4 whose weight dword holds w[c][r][4] in byte 0 and zeros above it;
//   * a transposed input row serves every output row of the tile that reads it (the row loop is unrolled, the rows of the
//     tile that a given input row feeds are known at compile time);
//   * the weights of the lane's 4 channels (R dwords per channel, 2R for 5x5) and the three tail constants per channel
//     (fq_int_tail.h: tail_consts / conv_tail_k) stay in registers while the lane walks its tiles: at most 2048 workgroups,
//     each lane strides over the tiles with its channel group fixed;
//   * neighbouring lanes are neighbouring channel groups of the same pixels, so 4 lanes cover 16 contiguous bytes and a
//     wave's load or store covers whole pixels; the column halo and the rows shared between bands are re-read from L1 / L2.
// Loads are predicated on the image bounds, stores on the output bounds; every offset is below N*H*W*Cpad / N*P*Q*Cpad
// (fq_dwconv_i8_geom.h, which scripts/dwconv_geom_check.cpp compiles as host code and walks over the test shapes).
// Channels [C, Cpad) are written as zeros whatever the input's padding channels hold: their tail constants are (0, 0, 0).
#include "fq_common.h"
#include "fq_int_tail.h"
#include "fq_dwconv_i8_geom.h"

namespace fq {

constexpr int kVarDepthwise = 14;      // fq_conv2d_i8_last_variant

struct DwParams {
    DwGeom g;
    int C;
    int rs, half_rs;                   // per-tensor shift (the per-channel form reads rs_k)
    int ilo, ihi, slo, shi;            // RightShift range, Sp range (slo = 0 with the fused ReLU)
};

// 4 pixels x 4 channels -> 4 channels x 4 pixels: t[c] = (d[0].byte c, d[1].byte c, d[2].byte c, d[3].byte c)
__device__ __forceinline__ void transpose4(const unsigned (&d)[4], unsigned (&t)[4]) {
    const unsigned a01 = __builtin_amdgcn_perm(d[1], d[0], 0x05010400u), b01 = __builtin_amdgcn_perm(d[1], d[0], 0x07030602u);
    const unsigned a23 = __builtin_amdgcn_perm(d[3], d[2], 0x05010400u), b23 = __builtin_amdgcn_perm(d[3], d[2], 0x07030602u);
    t[0] = __builtin_amdgcn_perm(a23, a01, 0x05040100u);
    t[1] = __builtin_amdgcn_perm(a23, a01, 0x07060302u);
    t[2] = __builtin_amdgcn_perm(b23, b01, 0x05040100u);
    t[3] = __builtin_amdgcn_perm(b23, b01, 0x07060302u);
}

template <int R, int STRIDE, bool PCS>
__global__ __launch_bounds__(kDwBlock) void dwconv_i8_kernel(const int8_t* __restrict__ x, const int8_t* __restrict__ w,
                                                            const float* __restrict__ qbias, const int32_t* __restrict__ rs_k,
                                                            int8_t* __restrict__ q, const DwParams p) {
    constexpr int S = R, TP = DwTile<R>::TP, TQ = kDwTQ;
    constexpr int NROWS = (TP - 1) * STRIDE + R;          // input rows of a tile
    constexpr int NPIX = (TQ - 1) * STRIDE + S;           // input columns of a tile
    constexpr int NG = (NPIX + 3) / 4;                    // transposed groups of 4 pixels
    const DwGeom& g = p.g;
    const unsigned gid = blockIdx.x * kDwBlock + threadIdx.x;
    const unsigned sp_stride = (gridDim.x * kDwBlock) / (unsigned)g.C4;
    const int c4 = (int)(gid % (unsigned)g.C4);
    unsigned tile = gid / (unsigned)g.C4;
    if (tile >= sp_stride) return;

    // this lane's weights: wr[r][c] = taps 0..3 of row r (byte s), w4[r][c] = tap 4 in byte 0 (5x5)
    unsigned wr[R][4], w4[S == 5 ? R : 1][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        unsigned d[4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
            d[s] = s < S ? *reinterpret_cast<const unsigned*>(w + (size_t)(r * S + s) * g.Cpad + 4 * c4) : 0u;
        transpose4(d, wr[r]);
        if constexpr (S == 5) {
            const unsigned d4 = *reinterpret_cast<const unsigned*>(w + (size_t)(r * S + 4) * g.Cpad + 4 * c4);
#pragma unroll
            for (int c = 0; c < 4; ++c) w4[r][c] = (d4 >> (8 * c)) & 0xffu;
        }
    }
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

    for (; tile < g.tiles; tile += sp_stride) {
        const DwTilePos tp = dw_tile_pos<TP>(g, tile);
        const int ih0 = tp.p0 * STRIDE - g.pad_h, iw0 = tp.q0 * STRIDE - g.pad_w;
        int acc[TP][4][TQ];
#pragma unroll
        for (int t = 0; t < TP; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int j = 0; j < TQ; ++j) acc[t][c][j] = 0;

#pragma unroll
        for (int i = 0; i < NROWS; ++i) {
            const int ih = ih0 + i;
            unsigned T[NG][4];
#pragma unroll
            for (int gg = 0; gg < NG; ++gg) {
                unsigned d[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int pix = 4 * gg + k, iw = iw0 + pix;
                    d[k] = 0u;
                    if (pix < NPIX && dw_in_ok(g, ih, iw)) d[k] = *reinterpret_cast<const unsigned*>(x + dw_in_off(g, tp.n, ih, iw, c4));
                }
                transpose4(d, T[gg]);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int j = 0; j < TQ; ++j) {
                    const int a = j * STRIDE;                 // first pixel of the window (compile time after unrolling)
                    const int ga = a / 4, oa = a % 4;
                    const unsigned win = oa == 0 ? T[ga][c] : __builtin_amdgcn_alignbyte(T[ga + (ga + 1 < NG ? 1 : 0)][c], T[ga][c], oa);
                    unsigned fifth = 0u;
                    if constexpr (S == 5) fifth = T[(a + 4) / 4][c] >> (8 * ((a + 4) % 4));
#pragma unroll
                    for (int t = 0; t < TP; ++t) {
                        const int r = i - t * STRIDE;         // the kernel row through which input row i reaches output row t
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
                const int pp = tp.p0 + t, qq = tp.q0 + j;
                if (dw_out_ok(g, pp, qq))
                    *reinterpret_cast<unsigned*>(q + dw_out_off(g, tp.n, pp, qq, c4)) = pack4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

static bool dw_supported(int C, int R, int S, int stride_h, int stride_w, int dil_h, int dil_w, int rs_min, int rs_max) {
    return C >= 1 && R == S && (R == 3 || R == 5) && stride_h == stride_w && (stride_h == 1 || stride_h == 2) && dil_h == 1 &&
           dil_w == 1 && rs_min >= 1 && rs_min <= rs_max && rs_max <= 16;
}

template <bool PCS>
static void dw_launch(int R, int stride, unsigned blocks, hipStream_t st, const int8_t* x, const int8_t* w, const float* qbias,
                      const int32_t* rs_k, int8_t* q, const DwParams& p) {
    if (R == 3 && stride == 1) dwconv_i8_kernel<3, 1, PCS><<<blocks, kDwBlock, 0, st>>>(x, w, qbias, rs_k, q, p);
    else if (R == 3) dwconv_i8_kernel<3, 2, PCS><<<blocks, kDwBlock, 0, st>>>(x, w, qbias, rs_k, q, p);
    else if (stride == 1) dwconv_i8_kernel<5, 1, PCS><<<blocks, kDwBlock, 0, st>>>(x, w, qbias, rs_k, q, p);
    else dwconv_i8_kernel<5, 2, PCS><<<blocks, kDwBlock, 0, st>>>(x, w, qbias, rs_k, q, p);
}

static int dwconv_dispatch(const int8_t* x_nhwc, const int8_t* w_rsc, const float* qbias, const int32_t* rs_k, int rs_min,
                           int rs_max, int8_t* q_nhwc, int Cpad, SpRange sp, int N, int H, int W, int C, int R, int S, int stride_h,
                           int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int ob, fq_stream_t stream) {
    if (!sp_range_valid(sp)) return FQ_ERR_INVALID_ARG;   // (the Sp range: [-128, 127], [0, 127] with a ReLU, or an _act caller's)
    if (rs_min < -120 || rs_max > 120 || rs_min > rs_max || ob < -120 || ob > 120) return FQ_ERR_INVALID_ARG;
    if (rs_k && (reinterpret_cast<uintptr_t>(rs_k) & 15u)) return FQ_ERR_INVALID_ARG;
    if (N < 0 || H <= 0 || W <= 0 || C <= 0 || R <= 0 || S <= 0 || stride_h <= 0 || stride_w <= 0 || pad_h < 0 || pad_w < 0 ||
        dil_h <= 0 || dil_w <= 0)
        return FQ_ERR_INVALID_ARG;
    if (Cpad % 16) return FQ_ERR_UNSUPPORTED;             // as fq_conv2d_i8_resident: pad channels to 16
    if (Cpad < C) return FQ_ERR_INVALID_ARG;
    if (!dw_supported(C, R, S, stride_h, stride_w, dil_h, dil_w, rs_min, rs_max) || pad_h >= R || pad_w >= S)
        return FQ_ERR_UNSUPPORTED;
    const int P = (H + 2 * pad_h - R) / stride_h + 1, Q = (W + 2 * pad_w - S) / stride_w + 1;
    if (H + 2 * pad_h < R || W + 2 * pad_w < S || P <= 0 || Q <= 0) return FQ_ERR_INVALID_ARG;
    g_last_conv_variant = kVarNone;
    if (N == 0) return FQ_OK;
    if (!x_nhwc || !w_rsc || !qbias || !q_nhwc) return FQ_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(x_nhwc) | reinterpret_cast<uintptr_t>(w_rsc) | reinterpret_cast<uintptr_t>(q_nhwc)) & 15u)
        return FQ_ERR_INVALID_ARG;
    // 32-bit element offsets into both activations; the channel groups of one pixel fit the launch
    if ((long)N * H * W * Cpad >= 0x7fffffffL || (long)N * P * Q * Cpad >= 0x3fffffffL || Cpad > 65536) return FQ_ERR_UNSUPPORTED;
    DwParams p;
    DwGeom& g = p.g;
    const int TP = R == 3 ? DwTile<3>::TP : DwTile<5>::TP;
    g.N = N; g.H = H; g.W = W; g.P = P; g.Q = Q; g.Cpad = Cpad; g.C4 = Cpad / 4; g.pad_h = pad_h; g.pad_w = pad_w;
    g.PB = (P + TP - 1) / TP; g.QB = (Q + kDwTQ - 1) / kDwTQ;
    const long tiles = (long)N * g.PB * g.QB;
    g.tiles = (unsigned)tiles;
    p.C = C;
    // accumulator bound of the integer tail (fq_int_tail.h): 25 * 128 * 128 < 2^19, bias term below 2^(9 + 16)
    p.rs = rs_min; p.half_rs = 1 << (rs_min - 1);
    // (any Sp range inside [-128, 127] keeps tail_consts' bias clamp inside [-255, 255])
    p.ilo = -128; p.ihi = 127; p.slo = sp.lo; p.shi = sp.hi;
    const long lanes = tiles * g.C4;
    long blocks = (lanes + kDwBlock - 1) / kDwBlock;
    if (blocks > kDwMaxBlocks) blocks = kDwMaxBlocks;
    hipStream_t st = as_stream(stream);
    if (rs_k) dw_launch<true>(R, stride_h, (unsigned)blocks, st, x_nhwc, w_rsc, qbias, rs_k, q_nhwc, p);
    else dw_launch<false>(R, stride_h, (unsigned)blocks, st, x_nhwc, w_rsc, qbias, nullptr, q_nhwc, p);
    note_conv_variant(kVarDepthwise, 0);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace fq

using namespace fq;

extern "C" int fq_dwconv2d_i8_supported(int C, int R, int S, int stride_h, int stride_w, int dil_h, int dil_w, int rs_min,
                                        int rs_max) {
    return dw_supported(C, R, S, stride_h, stride_w, dil_h, dil_w, rs_min, rs_max) ? 1 : 0;
}

extern "C" int fq_dwconv2d_i8_resident(const int8_t* x_nhwc, const int8_t* w_rsc, const float* qbias, int8_t* q_nhwc, int Cpad,
                                       int relu, int N, int H, int W, int C, int R, int S, int stride_h, int stride_w, int pad_h,
                                       int pad_w, int dil_h, int dil_w, int rs, int ob, fq_stream_t stream) {
    return dwconv_dispatch(x_nhwc, w_rsc, qbias, nullptr, rs, rs, q_nhwc, Cpad, sp_range_relu(relu), N, H, W, C, R, S, stride_h, stride_w, pad_h,
                           pad_w, dil_h, dil_w, ob, stream);
}

extern "C" int fq_dwconv2d_i8_resident_pcs(const int8_t* x_nhwc, const int8_t* w_rsc, const float* qbias, const int32_t* rs_k,
                                           int rs_min, int rs_max, int8_t* q_nhwc, int Cpad, int relu, int N, int H, int W, int C,
                                           int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                           int ob, fq_stream_t stream) {
    if (!rs_k && N > 0) return FQ_ERR_INVALID_ARG;
    return dwconv_dispatch(x_nhwc, w_rsc, qbias, rs_k, rs_min, rs_max, q_nhwc, Cpad, sp_range_relu(relu), N, H, W, C, R, S, stride_h, stride_w,
                           pad_h, pad_w, dil_h, dil_w, ob, stream);
}

extern "C" int fq_dwconv2d_i8_resident_act(const int8_t* x_nhwc, const int8_t* w_rsc, const float* qbias, int8_t* q_nhwc, int Cpad,
                                           int act_lo, int act_hi, int N, int H, int W, int C, int R, int S, int stride_h,
                                           int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int rs, int ob,
                                           fq_stream_t stream) {
    return dwconv_dispatch(x_nhwc, w_rsc, qbias, nullptr, rs, rs, q_nhwc, Cpad, SpRange{act_lo, act_hi}, N, H, W, C, R, S, stride_h,
                           stride_w, pad_h, pad_w, dil_h, dil_w, ob, stream);
}

extern "C" int fq_dwconv2d_i8_resident_pcs_act(const int8_t* x_nhwc, const int8_t* w_rsc, const float* qbias, const int32_t* rs_k,
                                               int rs_min, int rs_max, int8_t* q_nhwc, int Cpad, int act_lo, int act_hi, int N, int H,
                                               int W, int C, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w,
                                               int dil_h, int dil_w, int ob, fq_stream_t stream) {
    if (!rs_k && N > 0) return FQ_ERR_INVALID_ARG;
    return dwconv_dispatch(x_nhwc, w_rsc, qbias, rs_k, rs_min, rs_max, q_nhwc, Cpad, SpRange{act_lo, act_hi}, N, H, W, C, R, S,
                           stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, ob, stream);
}
