// fq_gconv_f32.hip -- the grouped (1 < groups, at least 4 channels per group: ResNeXt, RegNet, ShuffleNet) float convolutions
// of the calibration forward (include/fq.h: fq_gconv_f32), with the calibration's statistic taken in the epilogue, as
// fq_conv1x1_f32.hip does for the dense layers and fq_dwconv_f32.hip for the depthwise ones.
//
//   y[n][k][oh][ow] = bias[k] + sum_{r,s,c} w[k][c][r][s] * x[n][g Cgi + c][oh*stride - pad + r][ow*stride - pad + s]   (fp32 NCHW)
//   with g = k / Cgo, c over the Cgi input channels of the group.
//
// One form, on the vector ALU, for every channel count per group (4 .. 64):
//   * a tile is one (image, group, chunk of KC output channels, row band, column block) (fq_gconv_f32_geom.h: gf_plan); the
//     group's Cgi input windows, zero halo included, are staged in LDS by the whole workgroup -- consecutive lanes load
//     consecutive floats of an input row.  A pixel outside the image is the operand +0.0f in LDS: no value of a neighbouring
//     row, plane or group is ever loaded for it and no product is masked;
//   * the chunk's weights are staged in front of the input as [tap][c][KC] (read from w_kcrs in its own order, a contiguous
//     run), the chunk's bias behind them; the input takes the rest of the workgroup's 52 KB, so a group of few channels gets
//     tall tiles;
//   * a lane owns a 1 x 4 output strip of 4 consecutive output channels: 16 accumulators, each ONE fmaf chain over (r, s, c)
//     with c innermost, from +0.0f.  Per (r, s, c) it reads the floats under the strip as 16-byte LDS reads and its 4 weights as
//     one 16-byte LDS read (the lanes of a wave mostly share it: a broadcast); then the bias, the statistic and one 16-byte
//     store per channel where the address allows;
//   * at most 2048 workgroups (1024 in the histogram form, which flushes 2048 bins per workgroup), each walking its tiles.
//
// Numerics: one chain per output whatever N, the tile or the lane is -- every form of the kernel stores the same bits, and
// image i of a batch gets the bits of the same image alone.  No split, no workspace, no float atomics but publish_max's.
#include "fq_common.h"
#include "fq_producer_stat.h"
#include "fq_gconv_f32_geom.h"

namespace fq {
namespace {

constexpr int kT = kGfBlock;
typedef float f4v __attribute__((ext_vector_type(4)));

struct GfArgs {
    const float* x;
    const float* w;                    // [K][Cgi][R][S]: the module's own weight
    const float* bias;                 // [K] or null
    float* y;                          // or null (relu given)
    float* relu;                       // or null
    GfGeom g;
};

template <int R, int STRIDE, typename Stat>
__device__ __forceinline__ void gf_tiles(const GfArgs& a, Stat& stat, float* smem) {
    constexpr int NRD = ((kGfStrip - 1) * STRIDE + R + 3) / 4;    // 16-byte LDS reads per strip and kernel row
    const GfGeom& g = a.g;
    float* const s_w = smem;                                      // [RR][Cgi][KC]
    float* const s_b = smem + g.b0;                               // [KC]
    float* const s_x = smem + g.x0;                               // [Cgi][IH][IWP]: everything behind the weights and the bias
    const unsigned tid = threadIdx.x;
    const GfLanePos lp = gf_lane_pos(g, tid);
    const unsigned rd0 = lp.active ? gf_read_index(g, lp) : 0u;
    const unsigned wr0 = lp.active ? gf_w_index(g, lp, 0, 0) : 0u;
    const int Cgi = g.Cgi, KC = g.KC;
    const unsigned slot = g.slot;

    for (unsigned tile = geom_first_tile(blockIdx.x, gridDim.x); tile < g.tiles; tile += gridDim.x) {
        const GfTilePos tp = gf_tile_pos(g, tile);
        // stage the input: four loads in flight per lane, then their LDS stores
        for (unsigned e0 = tid; e0 < g.fill; e0 += 4u * kT) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned e = e0 + (unsigned)j * kT;
                unsigned off = 0;
                const bool ld = e < g.fill && gf_fill_src(g, tp, e, &off);
                v[j] = 0.0f;
                if (ld) v[j] = a.x[off];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned e = e0 + (unsigned)j * kT;
                if (e < g.fill) s_x[e] = v[j];
            }
        }
        // the chunk's weights and bias
        for (unsigned i0 = tid; i0 < g.wfill; i0 += 4u * kT) {
            float v[4];
            unsigned dst[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned i = i0 + (unsigned)j * kT;
                unsigned off = 0;
                dst[j] = 0;
                const bool ld = i < g.wfill && gf_w_src(g, tp, i, &off, &dst[j]);
                v[j] = 0.0f;
                if (ld) v[j] = a.w[off];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + (unsigned)j * kT < g.wfill) s_w[dst[j]] = v[j];
        }
        if (tid < (unsigned)KC) {
            const int k = tp.k0 + (int)tid;
            s_b[tid] = (a.bias && k < g.Cgo) ? a.bias[tp.grp * (unsigned)g.Cgo + (unsigned)k] : 0.0f;
        }
        __syncthreads();

        const int cnt = gf_out_count(g, tp, lp);
        if (cnt > 0) {
            float acc[kGfKB][kGfStrip];
#pragma unroll
            for (int kk = 0; kk < kGfKB; ++kk)
#pragma unroll
                for (int j = 0; j < kGfStrip; ++j) acc[kk][j] = 0.0f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int s = 0; s < R; ++s) {
                    const float* xp = s_x + rd0 + (unsigned)(r * g.IWP);
                    const float* wp = s_w + wr0 + (unsigned)((r * R + s) * Cgi * KC);
#pragma unroll 4
                    for (int c = 0; c < Cgi; ++c) {
                        const f4v* row = reinterpret_cast<const f4v*>(xp);
                        float in[4 * NRD];
#pragma unroll
                        for (int q = 0; q < NRD; ++q) {
                            const f4v t = row[q];
                            in[4 * q] = t[0]; in[4 * q + 1] = t[1]; in[4 * q + 2] = t[2]; in[4 * q + 3] = t[3];
                        }
                        const f4v wv = *reinterpret_cast<const f4v*>(wp);
#pragma unroll
                        for (int kk = 0; kk < kGfKB; ++kk)
#pragma unroll
                            for (int j = 0; j < kGfStrip; ++j) acc[kk][j] = __builtin_fmaf(wv[kk], in[j * STRIDE + s], acc[kk][j]);
                        xp += slot;
                        wp += KC;
                    }
                }
            }
            const f4v bv = *reinterpret_cast<const f4v*>(s_b + lp.kb * kGfKB);
#pragma unroll
            for (int kk = 0; kk < kGfKB; ++kk) {
                const unsigned o = gf_out_off(g, tp, lp, kk);
                float out[kGfStrip], rl[kGfStrip];
#pragma unroll
                for (int j = 0; j < kGfStrip; ++j) {
                    const float val = acc[kk][j] + bv[kk];
                    out[j] = stat_map(stat, val);
                    rl[j] = relu_like_torch(val);
                    if (j < cnt) stat.add(val);
                }
                if (a.y) {
                    float* p = a.y + o;
                    if (cnt == kGfStrip && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
                        *reinterpret_cast<f4v*>(p) = f4v{out[0], out[1], out[2], out[3]};
                    } else {
#pragma unroll
                        for (int j = 0; j < kGfStrip; ++j)
                            if (j < cnt) p[j] = out[j];
                    }
                }
                if (a.relu) {
                    float* p = a.relu + o;
                    if (cnt == kGfStrip && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
                        *reinterpret_cast<f4v*>(p) = f4v{rl[0], rl[1], rl[2], rl[3]};
                    } else {
#pragma unroll
                        for (int j = 0; j < kGfStrip; ++j)
                            if (j < cnt) p[j] = rl[j];
                    }
                }
            }
        }
        __syncthreads();                                          // the next tile overwrites the staged input and weights
    }
}

template <int R, int STRIDE, typename Stat>
__global__ __launch_bounds__(kT) void gconv_f32_kernel(const GfArgs a, const ProducerStatArgs sa) {
    __shared__ __attribute__((aligned(16))) float smem[kGfLdsFloats];
    if constexpr (__is_same(Stat, HistTag)) {
        __shared__ unsigned int s_bins[FQ_BINS + kWave];
        for (int b = threadIdx.x; b < FQ_BINS + kWave; b += kT) s_bins[b] = 0u;
        __syncthreads();
        const float iv = *sa.interval;
        unsigned int* park = s_bins + FQ_BINS + (threadIdx.x & (kWave - 1));
        if (sa.allow_fast && fast_quotient_ok(iv)) {
            HistStat<true> st{s_bins, park, iv, 1.0f / iv};
            gf_tiles<R, STRIDE>(a, st, smem);
        } else {
            HistStat<false> st{s_bins, park, iv, 1.0f / iv};
            gf_tiles<R, STRIDE>(a, st, smem);
        }
        hist_flush<kT>(s_bins, sa.hist_row);
    } else if constexpr (__is_same(Stat, MaxStat)) {
        MaxStat st;
        gf_tiles<R, STRIDE>(a, st, smem);
        publish_max<kT>(st.m, sa.max_bits);
    } else if constexpr (__is_same(Stat, QdStat)) {
        QdStat st = sa.qd;
        gf_tiles<R, STRIDE>(a, st, smem);
    } else {
        NoStat st;
        gf_tiles<R, STRIDE>(a, st, smem);
    }
}

template <typename Stat>
void gf_launch(int R, int stride, unsigned grid, hipStream_t st, const GfArgs& a, const ProducerStatArgs& sa) {
    if (R == 3 && stride == 1) hipLaunchKernelGGL((gconv_f32_kernel<3, 1, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
    else if (R == 3) hipLaunchKernelGGL((gconv_f32_kernel<3, 2, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
    else if (stride == 1) hipLaunchKernelGGL((gconv_f32_kernel<1, 1, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
    else hipLaunchKernelGGL((gconv_f32_kernel<1, 2, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
}

int gf_dispatch(const float* x, const float* w, const float* bias, float* y, float* relu_out, int N, int C, int H, int W, int K,
                int groups, int R, int S, int stride, int pad, float* max_inout, const float* interval, int64_t* hist_row,
                const QdStat* qd, fq_stream_t stream) {
    if (N < 1 || C < 1 || H < 1 || W < 1 || K < 1 || groups < 1 || R < 1 || S < 1 || stride < 1 || pad < 0) return FQ_ERR_INVALID_ARG;
    if (const int rc = producer_args_ok(x, w, bias, y, relu_out, max_inout, interval, hist_row, qd)) return rc;
    if (!gf_supported(C, K, groups, R, S, stride, stride, pad, pad, 1, 1, H, W)) return FQ_ERR_UNSUPPORTED;
    const long Ho = (H + 2 * pad - R) / stride + 1, Wo = (W + 2 * pad - S) / stride + 1;
    // 32-bit element offsets into x, y and w
    if ((long)N * C * H * W >= (1L << 30) || (long)N * K * Ho * Wo >= (1L << 30) || (long)K * (C / groups) * R * S >= (1L << 30))
        return FQ_ERR_UNSUPPORTED;
    GfArgs a;
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.relu = relu_out;
    if (!gf_plan(a.g, N, C, H, W, K, groups, R, stride, pad)) return FQ_ERR_UNSUPPORTED;
    ProducerStatArgs sa;
    sa.max_bits = reinterpret_cast<unsigned int*>(max_inout);
    sa.interval = interval;
    sa.hist_row = reinterpret_cast<unsigned long long*>(hist_row);
    sa.allow_fast = hist_fast_quotient_allowed();
    sa.qd = qd ? *qd : QdStat{1.0f, 1.0f, -128.0f, 127.0f};
    hipStream_t st = as_stream(stream);
    const unsigned grid = gf_grid(a.g, hist_row != nullptr);
    if (qd) gf_launch<QdStat>(R, stride, grid, st, a, sa);
    else if (hist_row) gf_launch<HistTag>(R, stride, grid, st, a, sa);
    else if (max_inout) gf_launch<MaxStat>(R, stride, grid, st, a, sa);
    else gf_launch<NoStat>(R, stride, grid, st, a, sa);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace
}  // namespace fq

using namespace fq;

extern "C" int fq_gconv_f32_supported(int C, int K, int groups, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w,
                                      int dil_h, int dil_w, int H, int W) {
    return gf_supported(C, K, groups, R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, H, W) ? 1 : 0;
}

extern "C" int fq_gconv_f32(const float* x, const float* w_kcrs, const float* bias, float* y, float* relu_out, int N, int C, int H,
                            int W, int K, int groups, int R, int S, int stride, int pad, float* max_inout, const float* interval,
                            int64_t* hist_row, fq_stream_t stream) {
    return gf_dispatch(x, w_kcrs, bias, y, relu_out, N, C, H, W, K, groups, R, S, stride, pad, max_inout, interval, hist_row, nullptr,
                       stream);
}

// TestConv.forward of a grouped layer in one kernel: QuanDequan(bit) of the value fq_gconv_f32 would have stored
extern "C" int fq_gconv_qd_f32(const float* x, const float* w_kcrs, const float* bias, float* y, int N, int C, int H, int W, int K,
                               int groups, int R, int S, int stride, int pad, int bit, int bitwidth, fq_stream_t stream) {
    QdStat qd;
    if (!qd_from_bit(bit, bitwidth, &qd)) return FQ_ERR_INVALID_ARG;
    return gf_dispatch(x, w_kcrs, bias, y, nullptr, N, C, H, W, K, groups, R, S, stride, pad, nullptr, nullptr, nullptr, &qd, stream);
}
