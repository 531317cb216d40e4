// fq_producer_stat.h -- what a producer kernel does with each output value while it is still in registers: the running
// abs-max of calibration pass 1 (distribution_collector.py:70-78) or the 2048-bin histogram of pass 2
// (distribution_collector.py:127-135).  Shared by the elementwise producers (fq_ops.hip) and the fp32 1x1 convolution
// (fq_conv1x1_f32.hip), and by every other float convolution of the calibration forward: what rides on such a convolution's
// output -- nothing, the abs-max, the histogram, a ReLU copy, or QuanDequan -- is written here once.
#pragma once
#include "fq_common.h"
#include "fq_hist_bin.h"

namespace fq {

// torch's clamp_min(x, 0): NaN stays NaN.  "not (v <= 0)" is true for v > 0 AND for NaN: one v_cmp_nle_f32 + one v_cndmask
// (the obvious  v > 0 ? v : (v != v ? v : 0)  is two compares, a scalar or and the select -- and every vector instruction of an
// epilogue is time the matrix pipe does not get)
__device__ __forceinline__ float relu_like_torch(float v) { return !(v <= 0.0f) ? v : 0.0f; }
// torch's clamp(x, 0, cap) -- nn.ReLU6 is hardtanh(x, 0, 6) -- bit for bit: NaN stays NaN (fminf(fmaxf(.)) would lose it: "r > cap"
// is false for NaN and hands r on), -0 and everything below become +0, everything above cap (+inf too) becomes cap, and cap
// itself, its neighbours and the neighbours of 0 pass through untouched.  relu_like_torch, one compare and one select more.
__device__ __forceinline__ float relu6_like_torch(float v, float cap) {
    const float r = relu_like_torch(v);
    return r > cap ? cap : r;
}

struct NoStat {
    __device__ __forceinline__ void add(float) {}
};
struct HistTag {};                                            // the histogram form: HistStat<fast> or HistStat<slow>, chosen by the interval at run time

struct MaxStat {
    float m = 0.0f;
    __device__ __forceinline__ void add(float v) { m = fmaxf(m, fabsf(v)); }                  // fmaxf drops NaN
};

// TestConv / TestLinear (new_quantity_op.py:283-292, :248-256): QuanDequan(bit) of the convolution's value on its way out
// of the accumulator -- not a statistic, a map: the stored value is map(v).  Bit for bit fq_quandequan_f32's expression.
struct QdStat {
    float scale, inv, lo, hi;                                 // 2^bit, 2^-bit, the integer range of the bit width
    __device__ __forceinline__ void add(float) {}
    __device__ __forceinline__ float map(float v) const {
        const float q = rintf(v * scale);
        return (q < lo ? lo : (q > hi ? hi : q)) * inv;       // NaN fails both compares and passes through
    }
};
// host: the map of QuanDequan(bit) at a bit width; false for a bit width other than 8 / 16 or a bit outside [-120, 120]
inline bool qd_from_bit(int bit, int bitwidth, QdStat* qd) {
    if (!valid_bitwidth(bitwidth) || bit < -120 || bit > 120) return false;
    qd->scale = ldexpf(1.0f, bit); qd->inv = ldexpf(1.0f, -bit);
    qd->lo = bitwidth == 8 ? -128.0f : -32768.0f; qd->hi = bitwidth == 8 ? 127.0f : 32767.0f;
    return true;
}

template <typename S> __device__ __forceinline__ float stat_map(const S&, float v) { return v; }
__device__ __forceinline__ float stat_map(const QdStat& s, float v) { return s.map(v); }

// The activation of the copy a producer writes next to its output (relu_out) rides on the same object: stat_act(stat, v) is
// nn.ReLU's max(v, 0) for every statistic above, and nn.ReLU6's clamp(v, 0, cap) for the same statistic wrapped in Clipped<> --
// the `_act` entry points (include/fq.h) instantiate their kernels on Clipped<NoStat / MaxStat / HistStat<>>, every other kernel
// is instantiated as before.  The statistic itself is untouched: it is taken from the UNCLIPPED value, as the hook on the
// convolution sees it.
template <typename S>
struct Clipped : S {
    float cap;
};
template <typename S> __device__ __forceinline__ float stat_act(const S&, float v) { return relu_like_torch(v); }
template <typename S> __device__ __forceinline__ float stat_act(const Clipped<S>& s, float v) { return relu6_like_torch(v, s.cap); }
// host: a cap an `_act` entry point accepts (positive and finite; nn.ReLU6: 6)
inline bool act_cap_ok(float cap) { return cap > 0.0f && cap <= 3.0e38f; }

template <bool kFast>
struct HistStat {
    unsigned int* bins;                                       // 2048 LDS counters of this workgroup
    unsigned int* park;                                       // exact zeros are not counted: a per-lane scratch slot
    float iv, yr;
    __device__ __forceinline__ void add(float v) { atomicAdd((v != 0.0f) ? (bins + bin_of<kFast>(v, iv, yr)) : park, 1u); }
};

// wave maximum -> LDS -> one atomicMax per workgroup on the non-negative float's bit pattern, and only when it can raise it
template <int kThreads>
__device__ __forceinline__ void publish_max(float m, unsigned int* __restrict__ max_bits) {
    __shared__ float s_wave[kThreads / kWave];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) s_wave[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kThreads / kWave; ++w) m = fmaxf(m, s_wave[w]);
        const unsigned int bits = __float_as_uint(m);
        if (bits > __hip_atomic_load(max_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(max_bits, bits);
    }
}

template <int kThreads>
__device__ __forceinline__ void hist_flush(unsigned int* s_bins, unsigned long long* __restrict__ dst) {
    __syncthreads();
    for (int b = threadIdx.x; b < FQ_BINS; b += kThreads) {
        const unsigned int c = s_bins[b];
        if (c) atomicAdd(dst + b, (unsigned long long)c);
    }
}

// what a producer kernel's launch carries for whichever statistic it was instantiated on
struct ProducerStatArgs {
    unsigned int* max_bits;
    const float* interval;
    unsigned long long* hist_row;
    int allow_fast;
    QdStat qd;
};

// host: the pointer rules the producers share -- one statistic at most, an interval with the histogram, y unless only the ReLU
// copy is wanted (never with QuanDequan), 4-byte aligned floats and an 8-byte aligned histogram row
inline int producer_args_ok(const float* x, const float* w, const float* bias, const float* y, const float* relu_out,
                            const float* max_inout, const float* interval, const int64_t* hist_row, const QdStat* qd) {
    if (max_inout && hist_row) return FQ_ERR_INVALID_ARG;
    if (hist_row && !interval) return FQ_ERR_INVALID_ARG;
    if (!x || !w || (!y && (!relu_out || qd))) return FQ_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(y) |
         reinterpret_cast<uintptr_t>(relu_out) | reinterpret_cast<uintptr_t>(max_inout) | reinterpret_cast<uintptr_t>(interval)) & 3u)
        return FQ_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(hist_row) & 7u) return FQ_ERR_INVALID_ARG;
    return FQ_OK;
}

}  // namespace fq
