// fq_dwconv_f32.hip -- the depthwise float convolutions of the calibration forward (include/fq.h: fq_dwconv_f32), with the
// calibration's statistic taken in the epilogue, as fq_conv1x1_f32.hip does for the dense layers.
//
//   y[n][c][oh][ow] = bias[c] + sum_{r,s} w[c][r][s] * x[n][c][oh*stride - pad + r][ow*stride - pad + s]       (fp32 NCHW)
//
// No sum over channels, so no matrix core and no reuse beyond the R x S window: 8 bytes of HBM traffic per output next to
// 9 or 25 multiply-adds.  The kernel is a copy with a stencil in the middle:
//   * a tile is PP plane slots of TH output rows x 4 QW output columns (fq_dwconv_f32_geom.h: dwf_plan); its input rows, zero
//     halo included, are staged in LDS by the whole workgroup -- consecutive lanes load consecutive floats of an input row, and
//     where a plane fits one tile the PP planes of the tile are ONE contiguous run of x (18 planes of 7 x 7, 4 of 14 x 14:
//     a 256-lane workgroup never works on 49 outputs).  A pixel outside the image is the operand +0.0f in LDS: no value of a
//     neighbouring row or plane is ever loaded for it and no product is masked;
//   * a lane owns one 1 x 4 output strip: per kernel row it reads the 3 stride + R floats under the strip as 16-byte LDS reads
//     (NCHW rows of 7, 14 or 28 floats are not 16-byte aligned in memory; the staged rows are) and runs the four fmaf chains,
//     r outer, s inner, from 0; then the bias, the statistic, and ONE 16-byte store per lane where the address allows --
//     the lanes of a tile row store a contiguous row segment;
//   * the R x S weights and the bias of the tile's planes are staged next to the input and read into registers once per tile;
//   * at most 2048 workgroups (1024 in the histogram form, which flushes 2048 bins per workgroup), each walking its tiles.
// Row-band halos (2 or 4 rows of a 16- to 18-row band) are re-read by the neighbouring tile, which an XCD's run of
// consecutive tiles (geom_first_tile) keeps in one L2.
//
// Numerics: one chain per output whatever N, the tile or the lane is -- every form of the kernel stores the same bits, and
// image i of a batch gets the bits of the same image alone.  No split, no workspace, no float atomics but publish_max's.
#include "fq_common.h"
#include "fq_producer_stat.h"
#include "fq_dwconv_f32_geom.h"

namespace fq {
namespace {

constexpr int kT = kDwfBlock;
typedef float f4v __attribute__((ext_vector_type(4)));

struct DwfArgs {
    const float* x;
    const float* w;                    // [C][R][S]: the module's own weight
    const float* bias;                 // [C] or null
    float* y;                          // or null (relu given)
    float* relu;                       // or null
    unsigned C;
    DwfGeom g;
};

template <int R, int STRIDE, typename Stat>
__device__ __forceinline__ void dwf_tiles(const DwfArgs& a, Stat& stat, float* smem) {
    constexpr int RR = R * R, WS = RR + 1;                        // a slot's weights and its bias
    constexpr int NRD = ((kDwfStrip - 1) * STRIDE + R + 3) / 4;   // 16-byte LDS reads per strip and kernel row
    const DwfGeom& g = a.g;
    float* const s_w = smem + kDwfLdsFloats;                      // [PP][WS]
    const unsigned tid = threadIdx.x;
    const DwfLanePos lp = dwf_lane_pos(g, tid);
    const unsigned rd0 = lp.active ? dwf_read_index(g, lp) : 0u;
    const unsigned nw = (unsigned)g.PP * WS;

    for (unsigned tile = geom_first_tile(blockIdx.x, gridDim.x); tile < g.tiles; tile += gridDim.x) {
        const DwfTilePos tp = dwf_tile_pos(g, tile);
        // stage: four loads in flight per lane, then their LDS stores
        for (unsigned e0 = tid; e0 < g.fill; e0 += 4u * kT) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned e = e0 + (unsigned)j * kT;
                unsigned off = 0;
                const bool ld = e < g.fill && dwf_fill_src(g, tp, e, &off);
                v[j] = 0.0f;
                if (ld) v[j] = a.x[off];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned e = e0 + (unsigned)j * kT;
                if (e < g.fill) smem[e] = v[j];
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

        const int cnt = dwf_out_count(g, tp, lp);
        if (cnt > 0) {
            float wv[RR];
#pragma unroll
            for (int k = 0; k < RR; ++k) wv[k] = s_w[lp.pi * WS + k];
            const float b = s_w[lp.pi * WS + RR];
            float acc[kDwfStrip] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const f4v* row = reinterpret_cast<const f4v*>(smem + rd0 + (unsigned)(r * g.IWP));
                float in[4 * NRD];
#pragma unroll
                for (int q = 0; q < NRD; ++q) {
                    const f4v t = row[q];
                    in[4 * q] = t[0]; in[4 * q + 1] = t[1]; in[4 * q + 2] = t[2]; in[4 * q + 3] = t[3];
                }
#pragma unroll
                for (int s = 0; s < R; ++s)
#pragma unroll
                    for (int j = 0; j < kDwfStrip; ++j) acc[j] = __builtin_fmaf(wv[r * R + s], in[j * STRIDE + s], acc[j]);
            }
            const unsigned o = dwf_out_off(g, tp, lp);
            float out[kDwfStrip], rl[kDwfStrip];
#pragma unroll
            for (int j = 0; j < kDwfStrip; ++j) {
                const float val = acc[j] + b;
                out[j] = stat_map(stat, val);
                rl[j] = stat_act(stat, val);
                if (j < cnt) stat.add(val);
            }
            if (a.y) {
                float* p = a.y + o;
                if (cnt == kDwfStrip && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
                    *reinterpret_cast<f4v*>(p) = f4v{out[0], out[1], out[2], out[3]};
                } else {
#pragma unroll
                    for (int j = 0; j < kDwfStrip; ++j)
                        if (j < cnt) p[j] = out[j];
                }
            }
            if (a.relu) {
                float* p = a.relu + o;
                if (cnt == kDwfStrip && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
                    *reinterpret_cast<f4v*>(p) = f4v{rl[0], rl[1], rl[2], rl[3]};
                } else {
#pragma unroll
                    for (int j = 0; j < kDwfStrip; ++j)
                        if (j < cnt) p[j] = rl[j];
                }
            }
        }
        __syncthreads();                                          // the next tile overwrites the staged rows and weights
    }
}

template <int R, int STRIDE, typename Stat>
__global__ __launch_bounds__(kT) void dwconv_f32_kernel(const DwfArgs a, const ProducerStatArgs sa) {
    __shared__ __attribute__((aligned(16))) float smem[kDwfLdsFloats + kDwfMaxPP * (R * R + 1)];
    if constexpr (__is_same(Stat, HistTag)) {
        __shared__ unsigned int s_bins[FQ_BINS + kWave];
        for (int b = threadIdx.x; b < FQ_BINS + kWave; b += kT) s_bins[b] = 0u;
        __syncthreads();
        const float iv = *sa.interval;
        unsigned int* park = s_bins + FQ_BINS + (threadIdx.x & (kWave - 1));
        if (sa.allow_fast && fast_quotient_ok(iv)) {
            HistStat<true> st{s_bins, park, iv, 1.0f / iv};
            dwf_tiles<R, STRIDE>(a, st, smem);
        } else {
            HistStat<false> st{s_bins, park, iv, 1.0f / iv};
            dwf_tiles<R, STRIDE>(a, st, smem);
        }
        hist_flush<kT>(s_bins, sa.hist_row);
    } else if constexpr (__is_same(Stat, MaxStat)) {
        MaxStat st;
        dwf_tiles<R, STRIDE>(a, st, smem);
        publish_max<kT>(st.m, sa.max_bits);
    } else if constexpr (__is_same(Stat, QdStat)) {
        QdStat st = sa.qd;
        dwf_tiles<R, STRIDE>(a, st, smem);
    } else {
        NoStat st;
        dwf_tiles<R, STRIDE>(a, st, smem);
    }
}

// the same with the ReLU copy clipped at `cap` (fq_dwconv_f32_act): the statistic wrapped in Clipped<>
template <int R, int STRIDE, typename Stat>
__global__ __launch_bounds__(kT) void dwconv_f32_act_kernel(const DwfArgs a, const ProducerStatArgs sa, const float cap) {
    __shared__ __attribute__((aligned(16))) float smem[kDwfLdsFloats + kDwfMaxPP * (R * R + 1)];
    if constexpr (__is_same(Stat, HistTag)) {
        __shared__ unsigned int s_bins[FQ_BINS + kWave];
        for (int b = threadIdx.x; b < FQ_BINS + kWave; b += kT) s_bins[b] = 0u;
        __syncthreads();
        const float iv = *sa.interval;
        unsigned int* park = s_bins + FQ_BINS + (threadIdx.x & (kWave - 1));
        if (sa.allow_fast && fast_quotient_ok(iv)) {
            Clipped<HistStat<true>> st{{s_bins, park, iv, 1.0f / iv}, cap};
            dwf_tiles<R, STRIDE>(a, st, smem);
        } else {
            Clipped<HistStat<false>> st{{s_bins, park, iv, 1.0f / iv}, cap};
            dwf_tiles<R, STRIDE>(a, st, smem);
        }
        hist_flush<kT>(s_bins, sa.hist_row);
    } else if constexpr (__is_same(Stat, MaxStat)) {
        Clipped<MaxStat> st{{}, cap};
        dwf_tiles<R, STRIDE>(a, st, smem);
        publish_max<kT>(st.m, sa.max_bits);
    } else {
        Clipped<NoStat> st{{}, cap};
        dwf_tiles<R, STRIDE>(a, st, smem);
    }
}

template <typename Stat>
void dwf_launch_act(int R, int stride, unsigned grid, hipStream_t st, const DwfArgs& a, const ProducerStatArgs& sa, float cap) {
    if (R == 3 && stride == 1) hipLaunchKernelGGL((dwconv_f32_act_kernel<3, 1, Stat>), dim3(grid), dim3(kT), 0, st, a, sa, cap);
    else if (R == 3) hipLaunchKernelGGL((dwconv_f32_act_kernel<3, 2, Stat>), dim3(grid), dim3(kT), 0, st, a, sa, cap);
    else if (stride == 1) hipLaunchKernelGGL((dwconv_f32_act_kernel<5, 1, Stat>), dim3(grid), dim3(kT), 0, st, a, sa, cap);
    else hipLaunchKernelGGL((dwconv_f32_act_kernel<5, 2, Stat>), dim3(grid), dim3(kT), 0, st, a, sa, cap);
}

template <typename Stat>
void dwf_launch(int R, int stride, unsigned grid, hipStream_t st, const DwfArgs& a, const ProducerStatArgs& sa) {
    if (R == 3 && stride == 1) hipLaunchKernelGGL((dwconv_f32_kernel<3, 1, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
    else if (R == 3) hipLaunchKernelGGL((dwconv_f32_kernel<3, 2, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
    else if (stride == 1) hipLaunchKernelGGL((dwconv_f32_kernel<5, 1, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
    else hipLaunchKernelGGL((dwconv_f32_kernel<5, 2, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
}

bool dwf_supported(int C, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int H, int W) {
    return C >= 1 && H >= 1 && W >= 1 && R == S && (R == 3 || R == 5) && stride_h == stride_w && (stride_h == 1 || stride_h == 2) &&
           pad_h == pad_w && pad_h >= 0 && pad_h < R && dil_h == 1 && dil_w == 1 && H + 2 * pad_h >= R && W + 2 * pad_w >= S;
}

int dwf_dispatch(const float* x, const float* w, const float* bias, float* y, float* relu_out, int N, int C, int H, int W, int R, int S,
                 int stride, int pad, float* max_inout, const float* interval, int64_t* hist_row, const QdStat* qd, fq_stream_t stream,
                 const float* cap = nullptr) {
    // (cap: the `_act` entry point -- relu_out receives clamp(y, 0, *cap) instead of max(y, 0); no QuanDequan form)
    if (cap && (!relu_out || qd || !act_cap_ok(*cap))) return FQ_ERR_INVALID_ARG;
    if (N < 1 || C < 1 || H < 1 || W < 1 || R < 1 || S < 1 || stride < 1 || pad < 0) return FQ_ERR_INVALID_ARG;
    if (const int rc = producer_args_ok(x, w, bias, y, relu_out, max_inout, interval, hist_row, qd)) return rc;
    if (!dwf_supported(C, R, S, stride, stride, pad, pad, 1, 1, H, W)) return FQ_ERR_UNSUPPORTED;
    const long Ho = (H + 2 * pad - R) / stride + 1, Wo = (W + 2 * pad - S) / stride + 1;
    // 32-bit element offsets into x and y
    if ((long)N * C * H * W >= (1L << 30) || (long)N * C * Ho * Wo >= (1L << 30)) return FQ_ERR_UNSUPPORTED;
    DwfArgs a;
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.relu = relu_out; a.C = (unsigned)C;
    if (!dwf_plan(a.g, N, C, H, W, R, stride, pad)) return FQ_ERR_UNSUPPORTED;
    ProducerStatArgs sa;
    sa.max_bits = reinterpret_cast<unsigned int*>(max_inout);
    sa.interval = interval;
    sa.hist_row = reinterpret_cast<unsigned long long*>(hist_row);
    sa.allow_fast = hist_fast_quotient_allowed();
    sa.qd = qd ? *qd : QdStat{1.0f, 1.0f, -128.0f, 127.0f};
    hipStream_t st = as_stream(stream);
    const unsigned grid = dwf_grid(a.g, hist_row != nullptr);
    if (cap) {
        if (hist_row) dwf_launch_act<HistTag>(R, stride, grid, st, a, sa, *cap);
        else if (max_inout) dwf_launch_act<MaxStat>(R, stride, grid, st, a, sa, *cap);
        else dwf_launch_act<NoStat>(R, stride, grid, st, a, sa, *cap);
    } else if (qd) dwf_launch<QdStat>(R, stride, grid, st, a, sa);
    else if (hist_row) dwf_launch<HistTag>(R, stride, grid, st, a, sa);
    else if (max_inout) dwf_launch<MaxStat>(R, stride, grid, st, a, sa);
    else dwf_launch<NoStat>(R, stride, grid, st, a, sa);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace
}  // namespace fq

using namespace fq;

extern "C" int fq_dwconv_f32_supported(int C, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                       int H, int W) {
    return dwf_supported(C, R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, H, W) ? 1 : 0;
}

extern "C" int fq_dwconv_f32(const float* x, const float* w_crs, const float* bias, float* y, float* relu_out, int N, int C, int H,
                             int W, int R, int S, int stride, int pad, float* max_inout, const float* interval, int64_t* hist_row,
                             fq_stream_t stream) {
    return dwf_dispatch(x, w_crs, bias, y, relu_out, N, C, H, W, R, S, stride, pad, max_inout, interval, hist_row, nullptr, stream);
}

extern "C" int fq_dwconv_f32_act(const float* x, const float* w_crs, const float* bias, float* y, float* relu_out, float act_cap, int N,
                                 int C, int H, int W, int R, int S, int stride, int pad, float* max_inout, const float* interval,
                                 int64_t* hist_row, fq_stream_t stream) {
    return dwf_dispatch(x, w_crs, bias, y, relu_out, N, C, H, W, R, S, stride, pad, max_inout, interval, hist_row, nullptr, stream,
                        &act_cap);
}

// TestConv.forward of a depthwise layer in one kernel: QuanDequan(bit) of the value fq_dwconv_f32 would have stored
extern "C" int fq_dwconv_qd_f32(const float* x, const float* w_crs, const float* bias, float* y, int N, int C, int H, int W, int R,
                                int S, int stride, int pad, int bit, int bitwidth, fq_stream_t stream) {
    QdStat qd;
    if (!qd_from_bit(bit, bitwidth, &qd)) return FQ_ERR_INVALID_ARG;
    return dwf_dispatch(x, w_crs, bias, y, nullptr, N, C, H, W, R, S, stride, pad, nullptr, nullptr, nullptr, &qd, stream);
}
