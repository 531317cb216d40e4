// fq_conv_dil_f32.hip -- the atrous dense 3x3 float convolutions of the calibration forward (include/fq.h: fq_conv_dil_f32; the
// 3x3s of a dilated ResNet's layer3 / layer4 and the dense ASPP branches of DeepLabV3) on the fp32 matrix cores, with the
// calibration's statistic taken in the epilogue as fq_conv1x1_f32.hip does for the undilated layers.
//
//   y[n][k][p][q] = bias[k] + sum_{c,r,s} W[k][c][r][s] * x[n][c][p - pad + r d][q - pad + s d]            (fp32 NCHW, stride 1)
//
// Implicit GEMM on v_mfma_f32_32x32x2_f32, A = 32 output channels across lanes, B = 32 output pixels across lanes, k = two
// input channels (fq_conv_dil_f32_geom.h has the plan and every address):
//   * a tile is 32 MT output channels x a TH x TW rectangle of output pixels of one image, a pixel per lane of the four waves;
//     MT = 2 where that still leaves 512 tiles, else 1 -- there is no K split, so small batches of small planes get the smaller
//     tile instead;
//   * LIVE TAPS ONLY: tap row r is live iff [p0 - pad + r d, p0 - pad + r d + th) meets [0, H), columns alike, decided once per
//     tile from the rectangle alone in uniform code; the K loop, the staging of x and the staging of the weights run over live
//     taps only.  A tile of a plane smaller than d runs one tap, a tile in the middle of a large plane nine;
//   * x is read from global memory once per tile and chunk of 8 input channels and reused by every live tap and every output
//     channel of the tile.  Only pixels inside the image are staged, compacted along BOTH axes (slot = input + off[r]); a staged
//     pixel is its 8 channels at a pitch of 9 floats, so the lanes' staging stores and operand reads (neighbouring pixels) fall
//     into neighbouring banks.  A tap whose source lies outside the image reads the workgroup's zero pixel: a lane selects one of
//     nine LDS addresses computed once per tile, never a value; the chunk's channel is the read's immediate offset.  There are no
//     zero margins: with the columns compacted like the rows a margin would have to be d wide, and the per-lane address select
//     costs nothing in the K loop;
//   * the weights of a (live tap, chunk), [8][32 MT] out of fq_conv_kxk_f32's pack, are staged once per workgroup and shared by
//     its waves;
//   * the next chunk's global loads (x and weights) are issued into registers before the current chunk's MFMAs and stored to LDS
//     behind them: one LDS buffer, the loads still run under the matrix work.  At most two workgroups share a CU (VGPRs);
//   * the epilogue stores 32 neighbouring pixels of one channel per half-wave and instruction -- a 128-byte run where the tile is
//     32 columns wide -- with 4-byte stores: the accumulator layout puts pixels across lanes, so a lane never holds neighbouring
//     pixels and any float offset of y is as good as another;
//   * at most 2048 workgroups (1024 in the histogram form), each walking its tiles from geom_first_tile on.
//
// Numerics: the MFMA is bit for bit an fmaf chain over its k, so an output is ONE chain from +0.0f over (chunk of 8 channels,
// live tap (r, s) ascending, channel of the chunk ascending), then + bias -- whatever N, the tile or the lane is: every form of
// the kernel stores the same bits, and image i of a batch gets the bits of that image alone.  No split, no workspace, no float
// atomics but publish_max's.
#include "fq_common.h"
#include "fq_producer_stat.h"
#include "fq_conv_dil_f32_geom.h"

namespace fq {
namespace {

constexpr int kT = kCdBlock;
constexpr int kCdXFloats = kCdMaxPx * kCdPitch;
typedef float f16v __attribute__((ext_vector_type(16)));

struct CdArgs {
    const float* x;
    const float* wt;                   // [(r*3 + s)*Cin + c][Cout]
    const float* bias;                 // [Cout] or null
    float* y;                          // or null (relu given)
    float* relu;                       // or null
    CdGeom g;
};

template <int MT, typename Stat>
__device__ __forceinline__ void cd_tiles(const CdArgs& a, Stat& stat, float* smem) {
    constexpr int BM = 32 * MT;
    constexpr int WPT = kCdChunk * BM / kT;                       // weights per thread, tap and chunk
    const CdGeom& g = a.g;
    float* const s_x = smem + kCdZero;                            // [staged pixel][kCdPitch]
    float* const s_w = smem + kCdZero + kCdXFloats;               // [tap][kCdChunk][BM]
    const unsigned tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const unsigned l32 = lane & 31u, h = lane >> 5;
    const unsigned Cin = (unsigned)g.Cin, Cout = (unsigned)g.Cout, plane = (unsigned)(g.H * g.W);
    if (tid < (unsigned)kCdZero) smem[tid] = 0.0f;                // the zero pixel: written once, never staged over

    for (unsigned tile = geom_first_tile(blockIdx.x, gridDim.x); tile < g.tiles; tile += gridDim.x) {
        const CdTilePos tp = cd_tile_pos(g, tile);
        unsigned live = 0;                                        // bit r*3 + s
#pragma unroll
        for (int t = 0; t < 9; ++t)
            if (((tp.rows.live >> (t / 3)) & (tp.cols.live >> (t % 3)) & 1) != 0) live |= 1u << t;

        unsigned goff[kCdPxPerThread];                            // the pixels this thread stages, chunk after chunk
#pragma unroll
        for (int i = 0; i < kCdPxPerThread; ++i) {
            const unsigned px = tid + (unsigned)i * kT;
            goff[i] = px < tp.staged ? cd_stage_src(g, tp, px) : 0u;
        }
        const unsigned xbase = cd_x_plane(g, tp.n, 0u);
        unsigned wm[WPT], wc[WPT];                                // the weights this thread stages per live tap
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const unsigned idx = tid + (unsigned)j * kT;
            wc[j] = idx / BM;
            wm[j] = tp.m0 + idx % BM;
        }

        CdLanePos lp;
        const bool has = cd_lane_pos(g, tp, wave * 32u + l32, &lp);
        const bool active = cd_wave_active(g, tp, wave);          // (wave-uniform)
        unsigned addr[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) addr[t] = cd_read_index(g, tp, has, lp, t / 3, t % 3) + h;

        f16v acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mt][e] = 0.0f;

        float xr[kCdPxPerThread][kCdChunk], wr[9][WPT];
        auto load = [&](unsigned c0) {
#pragma unroll
            for (int i = 0; i < kCdPxPerThread; ++i) {
                const bool ok = tid + (unsigned)i * kT < tp.staged;
#pragma unroll
                for (int c = 0; c < kCdChunk; ++c) {
                    xr[i][c] = 0.0f;
                    if (ok) xr[i][c] = a.x[xbase + (c0 + (unsigned)c) * plane + goff[i]];
                }
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                if (!(live & (1u << t))) continue;                // (uniform)
#pragma unroll
                for (int j = 0; j < WPT; ++j) {
                    wr[t][j] = 0.0f;
                    if (wm[j] < Cout) wr[t][j] = a.wt[((unsigned)t * Cin + c0 + wc[j]) * Cout + wm[j]];
                }
            }
        };

        load(0u);
        for (unsigned c0 = 0; c0 < Cin; c0 += kCdChunk) {
            __syncthreads();                                      // the last chunk's (or tile's) operand reads are done
#pragma unroll
            for (int i = 0; i < kCdPxPerThread; ++i) {
                const unsigned px = tid + (unsigned)i * kT;
                if (px < tp.staged) {
#pragma unroll
                    for (int c = 0; c < kCdChunk; ++c) s_x[px * kCdPitch + c] = xr[i][c];
                }
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                if (!(live & (1u << t))) continue;
#pragma unroll
                for (int j = 0; j < WPT; ++j) s_w[t * (kCdChunk * BM) + tid + j * kT] = wr[t][j];
            }
            __syncthreads();
            if (c0 + kCdChunk < Cin) load(c0 + kCdChunk);         // in flight under the MFMAs below
            if (active) {
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    if (!(live & (1u << t))) continue;
#pragma unroll
                    for (int i = 0; i < kCdChunk / 2; ++i) {
                        const float bv = smem[addr[t] + 2 * i];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            const float av = s_w[(t * kCdChunk + 2 * i + (int)h) * BM + mt * 32 + (int)l32];
                            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[mt], 0, 0, 0);
                        }
                    }
                }
            }
        }

        if (active && has) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const unsigned k = tp.m0 + (unsigned)mt * 32u + cd_acc_row(e, h);
                    if (k < Cout) {
                        const float val = acc[mt][e] + (a.bias ? a.bias[k] : 0.0f);
                        const unsigned o = cd_out_off(g, tp.n, k, lp);
                        if (a.y) a.y[o] = stat_map(stat, val);
                        if (a.relu) a.relu[o] = stat_act(stat, val);
                        stat.add(val);
                    }
                }
            }
        }
    }
}

template <int MT>
constexpr int cd_lds_floats() { return kCdZero + kCdXFloats + 9 * kCdChunk * 32 * MT; }

template <int MT, typename Stat>
__global__ __launch_bounds__(kT) void conv_dil_f32_kernel(const CdArgs a, const ProducerStatArgs sa) {
    __shared__ __attribute__((aligned(16))) float smem[cd_lds_floats<MT>()];
    if constexpr (__is_same(Stat, HistTag)) {
        __shared__ unsigned int s_bins[FQ_BINS + kWave];
        for (int b = threadIdx.x; b < FQ_BINS + kWave; b += kT) s_bins[b] = 0u;
        __syncthreads();
        const float iv = *sa.interval;
        unsigned int* park = s_bins + FQ_BINS + (threadIdx.x & (kWave - 1));
        if (sa.allow_fast && fast_quotient_ok(iv)) {
            HistStat<true> st{s_bins, park, iv, 1.0f / iv};
            cd_tiles<MT>(a, st, smem);
        } else {
            HistStat<false> st{s_bins, park, iv, 1.0f / iv};
            cd_tiles<MT>(a, st, smem);
        }
        hist_flush<kT>(s_bins, sa.hist_row);
    } else if constexpr (__is_same(Stat, MaxStat)) {
        MaxStat st;
        cd_tiles<MT>(a, st, smem);
        publish_max<kT>(st.m, sa.max_bits);
    } else if constexpr (__is_same(Stat, QdStat)) {
        QdStat st = sa.qd;
        cd_tiles<MT>(a, st, smem);
    } else {
        NoStat st;
        cd_tiles<MT>(a, st, smem);
    }
}

// the same with the ReLU copy clipped at `cap` (fq_conv_dil_f32_act): the statistic wrapped in Clipped<>
template <int MT, typename Stat>
__global__ __launch_bounds__(kT) void conv_dil_f32_act_kernel(const CdArgs a, const ProducerStatArgs sa, const float cap) {
    __shared__ __attribute__((aligned(16))) float smem[cd_lds_floats<MT>()];
    if constexpr (__is_same(Stat, HistTag)) {
        __shared__ unsigned int s_bins[FQ_BINS + kWave];
        for (int b = threadIdx.x; b < FQ_BINS + kWave; b += kT) s_bins[b] = 0u;
        __syncthreads();
        const float iv = *sa.interval;
        unsigned int* park = s_bins + FQ_BINS + (threadIdx.x & (kWave - 1));
        if (sa.allow_fast && fast_quotient_ok(iv)) {
            Clipped<HistStat<true>> st{{s_bins, park, iv, 1.0f / iv}, cap};
            cd_tiles<MT>(a, st, smem);
        } else {
            Clipped<HistStat<false>> st{{s_bins, park, iv, 1.0f / iv}, cap};
            cd_tiles<MT>(a, st, smem);
        }
        hist_flush<kT>(s_bins, sa.hist_row);
    } else if constexpr (__is_same(Stat, MaxStat)) {
        Clipped<MaxStat> st{{}, cap};
        cd_tiles<MT>(a, st, smem);
        publish_max<kT>(st.m, sa.max_bits);
    } else {
        Clipped<NoStat> st{{}, cap};
        cd_tiles<MT>(a, st, smem);
    }
}

template <typename Stat>
void cd_launch_act(int MT, unsigned grid, hipStream_t st, const CdArgs& a, const ProducerStatArgs& sa, float cap) {
    if (MT == 1) hipLaunchKernelGGL((conv_dil_f32_act_kernel<1, Stat>), dim3(grid), dim3(kT), 0, st, a, sa, cap);
    else hipLaunchKernelGGL((conv_dil_f32_act_kernel<2, Stat>), dim3(grid), dim3(kT), 0, st, a, sa, cap);
}

template <typename Stat>
void cd_launch(int MT, unsigned grid, hipStream_t st, const CdArgs& a, const ProducerStatArgs& sa) {
    if (MT == 1) hipLaunchKernelGGL((conv_dil_f32_kernel<1, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
    else hipLaunchKernelGGL((conv_dil_f32_kernel<2, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
}

int cd_dispatch(const float* x, const float* wt, const float* bias, float* y, float* relu_out, int N, int Cin, int H, int W, int Cout,
                int dil, int pad, float* max_inout, const float* interval, int64_t* hist_row, const QdStat* qd, fq_stream_t stream,
                const float* cap = nullptr) {
    // (cap: the `_act` entry point -- relu_out receives clamp(y, 0, *cap) instead of max(y, 0); no QuanDequan form)
    if (cap && (!relu_out || qd || !act_cap_ok(*cap))) return FQ_ERR_INVALID_ARG;
    if (N < 1 || Cin < 1 || H < 1 || W < 1 || Cout < 1 || dil < 1 || pad < 0) return FQ_ERR_INVALID_ARG;
    if (const int rc = producer_args_ok(x, wt, bias, y, relu_out, max_inout, interval, hist_row, qd)) return rc;
    if (!cd_supported(Cin, Cout, 1, 3, 3, 1, 1, pad, pad, dil, dil, H, W)) return FQ_ERR_UNSUPPORTED;
    const long Ho = (long)H + 2 * pad - 2L * dil, Wo = (long)W + 2 * pad - 2L * dil;
    // 32-bit element offsets into x, y and wt
    if ((long)N * Cin * H * W >= (1L << 30) || (long)N * Cout * Ho * Wo >= (1L << 30) || 9L * Cin * Cout >= (1L << 30))
        return FQ_ERR_UNSUPPORTED;
    CdArgs a;
    a.x = x; a.wt = wt; a.bias = bias; a.y = y; a.relu = relu_out;
    if (!cd_plan(a.g, N, Cin, Cout, H, W, dil, pad)) return FQ_ERR_UNSUPPORTED;
    ProducerStatArgs sa;
    sa.max_bits = reinterpret_cast<unsigned int*>(max_inout);
    sa.interval = interval;
    sa.hist_row = reinterpret_cast<unsigned long long*>(hist_row);
    sa.allow_fast = hist_fast_quotient_allowed();
    sa.qd = qd ? *qd : QdStat{1.0f, 1.0f, -128.0f, 127.0f};
    hipStream_t st = as_stream(stream);
    const unsigned grid = cd_grid(a.g, hist_row != nullptr);
    const int MT = a.g.MT;
    if (cap) {
        if (hist_row) cd_launch_act<HistTag>(MT, grid, st, a, sa, *cap);
        else if (max_inout) cd_launch_act<MaxStat>(MT, grid, st, a, sa, *cap);
        else cd_launch_act<NoStat>(MT, grid, st, a, sa, *cap);
    } else if (qd) cd_launch<QdStat>(MT, grid, st, a, sa);
    else if (hist_row) cd_launch<HistTag>(MT, grid, st, a, sa);
    else if (max_inout) cd_launch<MaxStat>(MT, grid, st, a, sa);
    else cd_launch<NoStat>(MT, grid, st, a, sa);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}

}  // namespace
}  // namespace fq

using namespace fq;

extern "C" int fq_conv_dil_f32_supported(int Cin, int Cout, int groups, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w,
                                         int dil_h, int dil_w, int H, int W) {
    return cd_supported(Cin, Cout, groups, R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, H, W) ? 1 : 0;
}

extern "C" int fq_conv_dil_f32(const float* x, const float* wq, const float* bias, float* y, float* relu_out, int N, int Cin, int H,
                               int W, int Cout, int dil, int pad, float* max_inout, const float* interval, int64_t* hist_row,
                               fq_stream_t stream) {
    return cd_dispatch(x, wq, bias, y, relu_out, N, Cin, H, W, Cout, dil, pad, max_inout, interval, hist_row, nullptr, stream);
}

extern "C" int fq_conv_dil_f32_act(const float* x, const float* wq, const float* bias, float* y, float* relu_out, float act_cap, int N,
                                   int Cin, int H, int W, int Cout, int dil, int pad, float* max_inout, const float* interval,
                                   int64_t* hist_row, fq_stream_t stream) {
    return cd_dispatch(x, wq, bias, y, relu_out, N, Cin, H, W, Cout, dil, pad, max_inout, interval, hist_row, nullptr, stream,
                       &act_cap);
}

// TestConv.forward of an atrous dense layer in one kernel: QuanDequan(bit) of the value fq_conv_dil_f32 would have stored
extern "C" int fq_conv_dil_qd_f32(const float* x, const float* wq, const float* bias, float* y, int N, int Cin, int H, int W, int Cout,
                                  int dil, int pad, int bit, int bitwidth, fq_stream_t stream) {
    QdStat qd;
    if (!qd_from_bit(bit, bitwidth, &qd)) return FQ_ERR_INVALID_ARG;
    return cd_dispatch(x, wq, bias, y, nullptr, N, Cin, H, W, Cout, dil, pad, nullptr, nullptr, nullptr, &qd, stream);
}
