// fq_dwconv_dil_f32.hip -- the atrous depthwise float convolutions of the calibration forward (include/fq.h:
// fq_dwconv_dil_f32), the calibration twin of fq_dwconv2d_dil_i8_resident, with the statistic taken in the epilogue as
// fq_dwconv_f32.hip does for the dense depthwise layers.
//
//   y[n][c][p][q] = bias[c] + sum_{r,s} w[c][r][s] * x[n][c][p - pad + r d][q - pad + s d]                  (fp32 NCHW, stride 1)
//
// 8 bytes of HBM traffic per output next to 9 or 25 multiply-adds, like the dense kernel -- but a dense band with its halo
// would be a 50 x 50 tile for the 196 outputs of a 14 x 14 plane at d = 18, nearly all of it padding.  So:
//   * a tile is PP plane slots x a band of TH output rows x the output width (fq_dwconv_dil_f32_geom.h: ddf_plan).  Only input
//     rows inside the image are staged, compacted: the rows kernel row r needs for the band are one run, and the runs of the R
//     kernel rows are disjoint while TH < d and merge into one from TH >= d on.  A plane that fits is staged once, whole, and
//     the PP planes of the tile are one contiguous run of x.  The LDS footprint is the plane's, whatever d is;
//   * a staged row lies between zero margins, so a 1 x 4 window may hang over either edge of the image; a window that lies
//     wholly outside the image -- its row or its columns -- is read from the workgroup's one zero row.  A lane selects an LDS
//     ADDRESS, never a value: an out-of-image tap is the product w * +0.0f like any other;
//   * a lane owns a 1 x 4 output strip at a time and walks the tile's strips.  Per tap it reads the 4 floats at column
//     4 j - pad + s d, whose alignment class (s d - pad) mod 4 is the same for every lane and tile (DdfGeom::cls): class 0 is
//     one 16-byte LDS read, class 2 two 8-byte reads, an odd class four 4-byte reads -- the widest aligned read the class
//     allows, 16 bytes per lane and tap in every case and no rotate (DESIGN section 40 has the arithmetic).  The staged row under
//     (band row, r) is an add, a compare and a multiply-add per strip and kernel row: no division in the tap loop;
//   * the R x S weights and the bias of the tile's planes are staged next to the input;
//   * at most 2048 workgroups (1024 in the histogram form), each walking its tiles from geom_first_tile on.
//
// Numerics: one chain per output whatever N, the tile or the lane is -- every form of the kernel stores the same bits, and
// image i of a batch gets the bits of the same image alone.  No split, no workspace, no float atomics but publish_max's.
#include "fq_common.h"
#include "fq_producer_stat.h"
#include "fq_dwconv_dil_f32_geom.h"

namespace fq {
namespace {

constexpr int kT = kDdfBlock;
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

struct DdfArgs {
    const float* x;
    const float* w;                    // [C][R][S]: the module's own weight
    const float* bias;                 // [C] or null
    float* y;                          // or null (relu given)
    float* relu;                       // or null
    unsigned C;
    DdfGeom g;
};

__device__ __forceinline__ void ddf_store(float* p, const float (&v)[kDdfStrip], int cnt) {
    if (cnt == kDdfStrip && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        *reinterpret_cast<f4v*>(p) = f4v{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < kDdfStrip; ++j)
            if (j < cnt) p[j] = v[j];
    }
}

template <int R, typename Stat>
__device__ __forceinline__ void ddf_tiles(const DdfArgs& a, Stat& stat, float* smem) {
    constexpr int RR = R * R, WS = RR + 1;                        // a slot's weights and its bias
    const DdfGeom& g = a.g;
    float* const s_in = smem + kDdfZero;                          // [PP][NR][pitch], behind the zero row
    float* const s_w = smem + kDdfLdsFloats;                      // [PP][WS]
    const unsigned tid = threadIdx.x;
    const unsigned nw = (unsigned)g.PP * WS;
    if (tid < (unsigned)kDdfZero) smem[tid] = 0.0f;               // the zero row: written once, never staged over

    for (unsigned tile = geom_first_tile(blockIdx.x, gridDim.x); tile < g.tiles; tile += gridDim.x) {
        const DdfTilePos tp = ddf_tile_pos(g, tile);
        // stage: four loads in flight per lane, then their LDS stores
        for (unsigned e0 = tid; e0 < g.fill; e0 += 4u * kT) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned e = e0 + (unsigned)j * kT;
                unsigned off = 0;
                const bool ld = e < g.fill && ddf_fill_src(g, tp, e, &off);
                v[j] = 0.0f;
                if (ld) v[j] = a.x[off];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned e = e0 + (unsigned)j * kT;
                if (e < g.fill) s_in[e] = v[j];
            }
        }
        for (unsigned i = tid; i < nw; i += kT) {
            const unsigned pi = i / WS, k = i - pi * WS, plane = tp.plane0 + pi;
            float v = 0.0f;
            if (plane < g.planes) {
                const unsigned c = plane % a.C;
                if (k < (unsigned)RR) v = a.w[c * RR + k];
                else if (a.bias) v = a.bias[c];
            }
            s_w[i] = v;
        }
        __syncthreads();

        for (unsigned u = tid; u < g.strips; u += kT) {
            const DdfStripPos lp = ddf_strip_pos(g, u);
            const int cnt = ddf_out_count(g, tp, lp);
            if (cnt == 0) continue;
            int col[R];
#pragma unroll
            for (int s = 0; s < R; ++s) col[s] = ddf_win_col(g, tp, lp.q, s);
            const float* const wv = s_w + lp.pi * WS;
            float acc[kDdfStrip] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int row = ddf_row_off(g, tp, lp.t, r);
#pragma unroll
                for (int s = 0; s < R; ++s) {
                    const float* const p = smem + ddf_read_index(g, lp.pi, row, col[s], s);
                    float in[kDdfStrip];
                    if (g.cls[s] == 0) {                          // (uniform: a scalar branch)
                        const f4v t = *reinterpret_cast<const f4v*>(p);
                        in[0] = t[0]; in[1] = t[1]; in[2] = t[2]; in[3] = t[3];
                    } else if (g.cls[s] == 2) {
                        const f2v t0 = *reinterpret_cast<const f2v*>(p), t1 = *reinterpret_cast<const f2v*>(p + 2);
                        in[0] = t0[0]; in[1] = t0[1]; in[2] = t1[0]; in[3] = t1[1];
                    } else {
                        in[0] = p[0]; in[1] = p[1]; in[2] = p[2]; in[3] = p[3];
                    }
                    const float wk = wv[r * R + s];
#pragma unroll
                    for (int j = 0; j < kDdfStrip; ++j) acc[j] = __builtin_fmaf(wk, in[j], acc[j]);
                }
            }
            const float b = wv[RR];
            const unsigned o = ddf_out_off(g, tp, lp);
            float out[kDdfStrip], rl[kDdfStrip];
#pragma unroll
            for (int j = 0; j < kDdfStrip; ++j) {
                const float val = acc[j] + b;
                out[j] = stat_map(stat, val);
                rl[j] = stat_act(stat, val);
                if (j < cnt) stat.add(val);
            }
            if (a.y) ddf_store(a.y + o, out, cnt);
            if (a.relu) ddf_store(a.relu + o, rl, cnt);
        }
        __syncthreads();                                          // the next tile overwrites the staged rows and weights
    }
}

template <int R, typename Stat>
__global__ __launch_bounds__(kT) void dwconv_dil_f32_kernel(const DdfArgs a, const ProducerStatArgs sa) {
    __shared__ __attribute__((aligned(16))) float smem[kDdfLdsFloats + kDdfMaxPP * (R * R + 1)];
    if constexpr (__is_same(Stat, HistTag)) {
        __shared__ unsigned int s_bins[FQ_BINS + kWave];
        for (int b = threadIdx.x; b < FQ_BINS + kWave; b += kT) s_bins[b] = 0u;
        __syncthreads();
        const float iv = *sa.interval;
        unsigned int* park = s_bins + FQ_BINS + (threadIdx.x & (kWave - 1));
        if (sa.allow_fast && fast_quotient_ok(iv)) {
            HistStat<true> st{s_bins, park, iv, 1.0f / iv};
            ddf_tiles<R>(a, st, smem);
        } else {
            HistStat<false> st{s_bins, park, iv, 1.0f / iv};
            ddf_tiles<R>(a, st, smem);
        }
        hist_flush<kT>(s_bins, sa.hist_row);
    } else if constexpr (__is_same(Stat, MaxStat)) {
        MaxStat st;
        ddf_tiles<R>(a, st, smem);
        publish_max<kT>(st.m, sa.max_bits);
    } else if constexpr (__is_same(Stat, QdStat)) {
        QdStat st = sa.qd;
        ddf_tiles<R>(a, st, smem);
    } else {
        NoStat st;
        ddf_tiles<R>(a, st, smem);
    }
}

// the same with the ReLU copy clipped at `cap` (fq_dwconv_dil_f32_act): the statistic wrapped in Clipped<>
template <int R, typename Stat>
__global__ __launch_bounds__(kT) void dwconv_dil_f32_act_kernel(const DdfArgs a, const ProducerStatArgs sa, const float cap) {
    __shared__ __attribute__((aligned(16))) float smem[kDdfLdsFloats + kDdfMaxPP * (R * R + 1)];
    if constexpr (__is_same(Stat, HistTag)) {
        __shared__ unsigned int s_bins[FQ_BINS + kWave];
        for (int b = threadIdx.x; b < FQ_BINS + kWave; b += kT) s_bins[b] = 0u;
        __syncthreads();
        const float iv = *sa.interval;
        unsigned int* park = s_bins + FQ_BINS + (threadIdx.x & (kWave - 1));
        if (sa.allow_fast && fast_quotient_ok(iv)) {
            Clipped<HistStat<true>> st{{s_bins, park, iv, 1.0f / iv}, cap};
            ddf_tiles<R>(a, st, smem);
        } else {
            Clipped<HistStat<false>> st{{s_bins, park, iv, 1.0f / iv}, cap};
            ddf_tiles<R>(a, st, smem);
        }
        hist_flush<kT>(s_bins, sa.hist_row);
    } else if constexpr (__is_same(Stat, MaxStat)) {
        Clipped<MaxStat> st{{}, cap};
        ddf_tiles<R>(a, st, smem);
        publish_max<kT>(st.m, sa.max_bits);
    } else {
        Clipped<NoStat> st{{}, cap};
        ddf_tiles<R>(a, st, smem);
    }
}

template <typename Stat>
void ddf_launch_act(int R, unsigned grid, hipStream_t st, const DdfArgs& a, const ProducerStatArgs& sa, float cap) {
    if (R == 3) hipLaunchKernelGGL((dwconv_dil_f32_act_kernel<3, Stat>), dim3(grid), dim3(kT), 0, st, a, sa, cap);
    else hipLaunchKernelGGL((dwconv_dil_f32_act_kernel<5, Stat>), dim3(grid), dim3(kT), 0, st, a, sa, cap);
}

template <typename Stat>
void ddf_launch(int R, unsigned grid, hipStream_t st, const DdfArgs& a, const ProducerStatArgs& sa) {
    if (R == 3) hipLaunchKernelGGL((dwconv_dil_f32_kernel<3, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
    else hipLaunchKernelGGL((dwconv_dil_f32_kernel<5, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
}

bool ddf_supported(int C, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int H, int W) {
    return C >= 1 && R == S && stride_h == 1 && stride_w == 1 && pad_h == pad_w && dil_h == dil_w &&
           ddf_window_ok(R, dil_h, pad_h, H, W);
}

int ddf_dispatch(const float* x, const float* w, const float* bias, float* y, float* relu_out, int N, int C, int H, int W, int R, int S,
                 int dil, int pad, float* max_inout, const float* interval, int64_t* hist_row, const QdStat* qd, fq_stream_t stream,
                 const float* cap = nullptr) {
    // (cap: the `_act` entry point -- relu_out receives clamp(y, 0, *cap) instead of max(y, 0); no QuanDequan form)
    if (cap && (!relu_out || qd || !act_cap_ok(*cap))) return FQ_ERR_INVALID_ARG;
    if (N < 1 || C < 1 || H < 1 || W < 1 || R < 1 || S < 1 || dil < 1 || pad < 0) return FQ_ERR_INVALID_ARG;
    if (const int rc = producer_args_ok(x, w, bias, y, relu_out, max_inout, interval, hist_row, qd)) return rc;
    if (!ddf_supported(C, R, S, 1, 1, pad, pad, dil, dil, H, W)) return FQ_ERR_UNSUPPORTED;
    const long Ho = (long)H + 2 * pad - (long)dil * (R - 1), Wo = (long)W + 2 * pad - (long)dil * (S - 1);
    // 32-bit element offsets into x and y
    if ((long)N * C * H * W >= (1L << 30) || (long)N * C * Ho * Wo >= (1L << 30)) return FQ_ERR_UNSUPPORTED;
    DdfArgs a;
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.relu = relu_out; a.C = (unsigned)C;
    if (!ddf_plan(a.g, N, C, H, W, R, dil, pad)) return FQ_ERR_UNSUPPORTED;
    ProducerStatArgs sa;
    sa.max_bits = reinterpret_cast<unsigned int*>(max_inout);
    sa.interval = interval;
    sa.hist_row = reinterpret_cast<unsigned long long*>(hist_row);
    sa.allow_fast = hist_fast_quotient_allowed();
    sa.qd = qd ? *qd : QdStat{1.0f, 1.0f, -128.0f, 127.0f};
    hipStream_t st = as_stream(stream);
    const unsigned grid = ddf_grid(a.g, hist_row != nullptr);
    if (cap) {
        if (hist_row) ddf_launch_act<HistTag>(R, grid, st, a, sa, *cap);
        else if (max_inout) ddf_launch_act<MaxStat>(R, grid, st, a, sa, *cap);
        else ddf_launch_act<NoStat>(R, grid, st, a, sa, *cap);
    } else if (qd) ddf_launch<QdStat>(R, grid, st, a, sa);
    else if (hist_row) ddf_launch<HistTag>(R, grid, st, a, sa);
    else if (max_inout) ddf_launch<MaxStat>(R, grid, st, a, sa);
    else ddf_launch<NoStat>(R, grid, st, a, sa);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace
}  // namespace fq

using namespace fq;

extern "C" int fq_dwconv_dil_f32_supported(int C, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                           int H, int W) {
    return ddf_supported(C, R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, H, W) ? 1 : 0;
}

extern "C" int fq_dwconv_dil_f32(const float* x, const float* w_crs, const float* bias, float* y, float* relu_out, int N, int C, int H,
                                 int W, int R, int S, int dil, int pad, float* max_inout, const float* interval, int64_t* hist_row,
                                 fq_stream_t stream) {
    return ddf_dispatch(x, w_crs, bias, y, relu_out, N, C, H, W, R, S, dil, pad, max_inout, interval, hist_row, nullptr, stream);
}

extern "C" int fq_dwconv_dil_f32_act(const float* x, const float* w_crs, const float* bias, float* y, float* relu_out, float act_cap,
                                     int N, int C, int H, int W, int R, int S, int dil, int pad, float* max_inout,
                                     const float* interval, int64_t* hist_row, fq_stream_t stream) {
    return ddf_dispatch(x, w_crs, bias, y, relu_out, N, C, H, W, R, S, dil, pad, max_inout, interval, hist_row, nullptr, stream,
                        &act_cap);
}

// TestConv.forward of an atrous depthwise layer in one kernel: QuanDequan(bit) of the value fq_dwconv_dil_f32 would have stored
extern "C" int fq_dwconv_dil_qd_f32(const float* x, const float* w_crs, const float* bias, float* y, int N, int C, int H, int W, int R,
                                    int S, int dil, int pad, int bit, int bitwidth, fq_stream_t stream) {
    QdStat qd;
    if (!qd_from_bit(bit, bitwidth, &qd)) return FQ_ERR_INVALID_ARG;
    return ddf_dispatch(x, w_crs, bias, y, nullptr, N, C, H, W, R, S, dil, pad, nullptr, nullptr, nullptr, &qd, stream);
}
