// fq_dwconv_i8_lane.h -- what one lane of a depthwise int8 kernel does in registers, shared by the dense kernel
// (fq_dwconv_i8.hip) and the atrous one (fq_dwconv_dil_i8.hip): the 4 pixels x 4 channels transpose, the window step over
// transposed groups and the lane's weights.  Device code only; nothing here knows how pixels are addressed.  (The tail constants
// of the lane's channels are set up in each kernel: behind a function boundary their four small arrays went to scratch.)
#pragma once
#include "fq_int_tail.h"

namespace fq {

// 4 pixels x 4 channels -> 4 channels x 4 pixels: t[c] = (d[0].byte c, d[1].byte c, d[2].byte c, d[3].byte c)
__device__ __forceinline__ void transpose4(const unsigned (&d)[4], unsigned (&t)[4]) {
    const unsigned a01 = __builtin_amdgcn_perm(d[1], d[0], 0x05010400u), b01 = __builtin_amdgcn_perm(d[1], d[0], 0x07030602u);
    const unsigned a23 = __builtin_amdgcn_perm(d[3], d[2], 0x05010400u), b23 = __builtin_amdgcn_perm(d[3], d[2], 0x07030602u);
    t[0] = __builtin_amdgcn_perm(a23, a01, 0x05040100u);
    t[1] = __builtin_amdgcn_perm(a23, a01, 0x07060302u);
    t[2] = __builtin_amdgcn_perm(b23, b01, 0x05040100u);
    t[3] = __builtin_amdgcn_perm(b23, b01, 0x07060302u);
}

// The window step.  T[g] holds pixels 4g .. 4g + 3 of one channel of one (lattice) row.  The window of an output column is the
// four pixels from a = 4 * ga + oa on: dw_window(T[ga], T[ga + 1], oa); the fifth tap of a 5-wide row is the byte behind them:
// dw_fifth(T[(a + 4) / 4], (a + 4) % 4).  a is a compile-time value after unrolling.
__device__ __forceinline__ unsigned dw_window(unsigned lo, unsigned hi, int oa) {
    return oa == 0 ? lo : __builtin_amdgcn_alignbyte(hi, lo, oa);
}
__device__ __forceinline__ unsigned dw_fifth(unsigned t, int ob) { return t >> (8 * ob); }

// this lane's weights from w [R][S][Cpad]: wr[r][c] = taps 0..3 of row r (byte s), w4[r][c] = tap 4 in byte 0 (5x5)
template <int R, int NW4>
__device__ __forceinline__ void dw_lane_weights(const int8_t* __restrict__ w, int Cpad, int c4, unsigned (&wr)[R][4],
                                                unsigned (&w4)[NW4][4]) {
    constexpr int S = R;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        unsigned d[4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
            d[s] = s < S ? *reinterpret_cast<const unsigned*>(w + (size_t)(r * S + s) * Cpad + 4 * c4) : 0u;
        transpose4(d, wr[r]);
        if constexpr (S == 5) {
            const unsigned d4 = *reinterpret_cast<const unsigned*>(w + (size_t)(r * S + 4) * Cpad + 4 * c4);
#pragma unroll
            for (int c = 0; c < 4; ++c) w4[r][c] = (d4 >> (8 * c)) & 0xffu;
        }
    }
}

}  // namespace fq
