// fq_deconv_f32.hip -- the transposed float convolutions (nn.ConvTranspose2d, groups 1, dilation 1: the up-convolutions of a
// U-Net, pix2pix, DCGAN or LinkNet decoder) of the calibration forward on the fp32 matrix cores (include/fq.h: fq_deconv_f32),
// with the calibration's statistic taken in the epilogue, as fq_conv1x1_f32.hip does for the dense layers.
//
//   y[n][k][oh][ow] = bias[k] + sum_{r,s,c} w[c][k][r][s] * x[n][c][(oh + pad - r)/stride][(ow + pad - s)/stride]     (fp32 NCHW)
//   over the taps with (oh + pad - r) % stride == 0 and (ow + pad - s) % stride == 0.
//
// Sub-pixel phases (fq_deconv_f32_geom.h): the outputs of one ((oh + pad) mod stride, (ow + pad) mod stride) form a sub-grid
// on which the layer is a dense stride-1 correlation over the taps of that phase -- fq_conv_kxk_f32's GEMM with columns
// (n, sub-grid pixel), one input offset per tap, and no product with a stuffed zero.  v_mfma_f32_32x32x2_f32 takes
// B[k][j] with j across lanes 0..31: 32 consecutive sub-grid columns of one input row (a 128-byte run of an input plane, as in
// the 1x1 kernel), and A[i][k] with i across lanes: 32 consecutive output channels of one row of wt [(r*S + s)*Cin + c][Cout].
//
//   * a work item is one (row phase, 32 MW output channels, 32 NW columns); the four waves of the workgroup sit MW x NW
//     (4 x 1 from 128 channels on, 1 x 4 up to 32), so the waves of a workgroup share either the columns' x or the channels' wt
//     in L1; both operands go from global memory straight to the MFMA, 16 input channels (8 MFMAs) per batch of loads;
//   * a wave owns ALL `stride` column phases of its 32 columns: `stride` accumulator tiles.  Lane q then holds the `stride`
//     neighbouring floats of an output row and stores them as one 8- or 16-byte run where the address allows (stride 2 and 4;
//     DESIGN.md section 36 has the times of this form and of one 4-byte store per column phase, `stride` floats apart);
//   * a tap outside the image is the operand +0.0f in the B register: nothing is loaded for it and no product is masked;
//   * at most 2048 workgroups (1024 in the histogram form), each walking its work items.
//
// Numerics: the MFMA is bit for bit an fmaf chain over its k, so an output is ONE chain over (r, s, c) ascending from +0.0f,
// whatever N, the tile or the lane is: every form of the kernel stores the same bits.  No split, no workspace, no float
// atomics but publish_max's.
#include "fq_common.h"
#include "fq_producer_stat.h"
#include "fq_deconv_f32_geom.h"

namespace fq {
namespace {

constexpr int kT = kDcBlock;
typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));

struct DcArgs {
    const float* x;
    const float* wt;                   // [(r*S + s)*Cin + c][Cout]
    const float* bias;                 // [Cout] or null
    float* y;                          // or null (relu given)
    float* relu;                       // or null
    DcGeom g;
};

// stores the `cnt` (of ST) neighbouring floats v[0 .. cnt-1] at p: one run where all exist and the address allows
template <int ST>
__device__ __forceinline__ void dc_store_run(float* p, const float (&v)[ST], int cnt) {
    if constexpr (ST == 2) {
        if (cnt == 2 && (reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
            *reinterpret_cast<f2v*>(p) = f2v{v[0], v[1]};
            return;
        }
    }
    if constexpr (ST == 4) {
        if (cnt == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
            *reinterpret_cast<f4v*>(p) = f4v{v[0], v[1], v[2], v[3]};
            return;
        }
    }
#pragma unroll
    for (int cp = 0; cp < ST; ++cp)
        if (cp < cnt) p[cp] = v[cp];
}

template <int ST, typename Stat>
__device__ __forceinline__ void dc_items(const DcArgs& a, Stat& stat) {
    const DcGeom& g = a.g;
    const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const unsigned l32 = lane & 31u, h = lane >> 5;
    const unsigned wm = dc_wave_m(g, wave), wj = dc_wave_j(g, wave);
    const unsigned Cin = (unsigned)g.Cin, Cout = (unsigned)g.Cout, plane = g.plane_in;

    for (unsigned item = geom_first_tile(blockIdx.x, gridDim.x); item < g.items; item += gridDim.x) {
        const DcItemPos ip = dc_item_pos(g, item);
        const unsigned mbase = ip.m0 + wm;
        if (mbase >= Cout) continue;                                           // (wave-uniform: a partly filled channel tile)
        const DcColPos col = dc_col_pos(g, ip.rp, ip.j0 + wj + l32);
        const unsigned ka = mbase + l32;                                       // the output channel this lane loads weights of
        const bool ka_ok = ka < Cout;

        f16v acc[ST];
#pragma unroll
        for (int cp = 0; cp < ST; ++cp)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[cp][e] = 0.0f;

        for (int r = dc_first_tap(g, ip.rp); r < g.R; r += ST) {
#pragma unroll
            for (int cp = 0; cp < ST; ++cp) {
                for (int s = dc_first_tap(g, cp); s < g.S; s += ST) {
                    unsigned xoff = 0;
                    const bool ld = dc_tap_src(g, col, ip.rp, cp, r, s, &xoff);
                    const float* xp = a.x + xoff + h * plane;
                    const float* wp = a.wt + dc_w_off(g, r, s, h, ka_ok ? ka : 0u);
                    for (unsigned c0 = 0; c0 < Cin; c0 += 16u) {              // Cin % 16 == 0
                        float av[8], bv[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            av[i] = 0.0f;
                            bv[i] = 0.0f;
                            if (ka_ok) av[i] = wp[(size_t)(c0 + 2u * i) * Cout];
                            if (ld) bv[i] = xp[(size_t)(c0 + 2u * i) * plane];
                        }
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[cp] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[i], acc[cp], 0, 0, 0);
                    }
                }
            }
        }

        const int cnt = dc_out_count(g, col);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const unsigned k = mbase + dc_acc_row(e, h);
            if (k < Cout && cnt > 0) {
                const float b = a.bias ? a.bias[k] : 0.0f;
                const unsigned o = dc_out_off(g, col, ip.rp, k);
                float out[ST], rl[ST];
#pragma unroll
                for (int cp = 0; cp < ST; ++cp) {
                    const float val = acc[cp][e] + b;
                    out[cp] = val;
                    rl[cp] = stat_act(stat, val);
                    if (cp < cnt) stat.add(val);
                }
                if (a.y) dc_store_run<ST>(a.y + o, out, cnt);
                if (a.relu) dc_store_run<ST>(a.relu + o, rl, cnt);
            }
        }
    }
}

template <int ST, typename Stat>
__global__ __launch_bounds__(kT) void deconv_f32_kernel(const DcArgs a, const ProducerStatArgs sa) {
    if constexpr (__is_same(Stat, HistTag)) {
        __shared__ unsigned int s_bins[FQ_BINS + kWave];
        for (int b = threadIdx.x; b < FQ_BINS + kWave; b += kT) s_bins[b] = 0u;
        __syncthreads();
        const float iv = *sa.interval;
        unsigned int* park = s_bins + FQ_BINS + (threadIdx.x & (kWave - 1));
        if (sa.allow_fast && fast_quotient_ok(iv)) {
            HistStat<true> st{s_bins, park, iv, 1.0f / iv};
            dc_items<ST>(a, st);
        } else {
            HistStat<false> st{s_bins, park, iv, 1.0f / iv};
            dc_items<ST>(a, st);
        }
        hist_flush<kT>(s_bins, sa.hist_row);
    } else if constexpr (__is_same(Stat, MaxStat)) {
        MaxStat st;
        dc_items<ST>(a, st);
        publish_max<kT>(st.m, sa.max_bits);
    } else {
        NoStat st;
        dc_items<ST>(a, st);
    }
}

template <typename Stat>
void dc_launch(int stride, unsigned grid, hipStream_t st, const DcArgs& a, const ProducerStatArgs& sa) {
    if (stride == 1) hipLaunchKernelGGL((deconv_f32_kernel<1, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
    else if (stride == 2) hipLaunchKernelGGL((deconv_f32_kernel<2, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
    else if (stride == 3) hipLaunchKernelGGL((deconv_f32_kernel<3, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
    else hipLaunchKernelGGL((deconv_f32_kernel<4, Stat>), dim3(grid), dim3(kT), 0, st, a, sa);
}

}  // namespace
}  // namespace fq

using namespace fq;

extern "C" int fq_deconv_f32_supported(int Cin, int Cout, int groups, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w,
                                       int outpad_h, int outpad_w, int dil_h, int dil_w, int H, int W) {
    return dc_supported(Cin, Cout, groups, R, S, stride_h, stride_w, pad_h, pad_w, outpad_h, outpad_w, dil_h, dil_w, H, W) ? 1 : 0;
}

extern "C" int fq_deconv_f32(const float* x, const float* wt, const float* bias, float* y, float* relu_out, int N, int Cin, int Hin,
                             int Win, int Cout, int R, int S, int stride, int pad, int outpad, float* max_inout,
                             const float* interval, int64_t* hist_row, fq_stream_t stream) {
    if (N < 0 || Cin < 1 || Hin < 1 || Win < 1 || Cout < 1 || R < 1 || S < 1 || stride < 1 || pad < 0 || outpad < 0)
        return FQ_ERR_INVALID_ARG;
    if (const int rc = producer_args_ok(x, wt, bias, y, relu_out, max_inout, interval, hist_row, nullptr)) return rc;
    if (reinterpret_cast<uintptr_t>(wt) & 15u) return FQ_ERR_INVALID_ARG;
    if (!dc_supported(Cin, Cout, 1, R, S, stride, stride, pad, pad, outpad, outpad, 1, 1, Hin, Win)) return FQ_ERR_UNSUPPORTED;
    const long Ho = (long)(Hin - 1) * stride - 2L * pad + R + outpad, Wo = (long)(Win - 1) * stride - 2L * pad + S + outpad;
    // 32-bit element offsets into x, y and wt
    if ((long)N * Cin * Hin * Win >= (1L << 30) || (long)N * Cout * Ho * Wo >= (1L << 30) || (long)R * S * Cin * Cout >= (1L << 30))
        return FQ_ERR_UNSUPPORTED;
    if (N == 0) return FQ_OK;
    DcArgs a;
    a.x = x; a.wt = wt; a.bias = bias; a.y = y; a.relu = relu_out;
    if (!dc_plan(a.g, N, Cin, Hin, Win, Cout, R, S, stride, pad, outpad)) return FQ_ERR_UNSUPPORTED;
    ProducerStatArgs sa;
    sa.max_bits = reinterpret_cast<unsigned int*>(max_inout);
    sa.interval = interval;
    sa.hist_row = reinterpret_cast<unsigned long long*>(hist_row);
    sa.allow_fast = hist_fast_quotient_allowed();
    sa.qd = QdStat{1.0f, 1.0f, -128.0f, 127.0f};
    hipStream_t st = as_stream(stream);
    const unsigned grid = dc_grid(a.g, hist_row != nullptr);
    if (hist_row) dc_launch<HistTag>(stride, grid, st, a, sa);
    else if (max_inout) dc_launch<MaxStat>(stride, grid, st, a, sa);
    else dc_launch<NoStat>(stride, grid, st, a, sa);
    FQ_LAUNCH_CHECK();
    return FQ_OK;
}
