// fq_act_lut_i8_geom.h -- the index arithmetic of the int8 NHWC activation-by-table kernel (fq_act_lut_i8.hip), kept apart from
// the kernel so that the same functions compile as host code: scripts/act_lut_geom_check.cpp walks them over the shapes the GPU
// tests run and asserts that every byte a lane touches lies inside its tensor and that every output byte is written exactly once.
//
//   y[pix][c] = table[x[pix][c] + 128]     0 <= c < C
//             = 0                          C <= c < Cpad
//
// The tensor is one run of n = npix * Cpad bytes.  It is cut into CHUNKS of 16 bytes (one dwordx4 load and store per lane) and a
// TAIL of n % 16 bytes (only where Cpad is no multiple of 16; the project's padding never leaves one).  Pass p of a workgroup
// covers chunks [p * stride + block * kActLutBlock, + kActLutBlock), stride = blocks * kActLutBlock: the loop bound is the same
// for every lane of a workgroup (the lane-crossing lookup needs whole waves), a lane past the last chunk neither loads nor stores.
// The tail's bytes are taken by the first lanes of workgroup 0, one byte each.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define FQ_ACT_HD __host__ __device__ __forceinline__
#else
#define FQ_ACT_HD inline
#endif

namespace fq {

constexpr int kActLutBlock = 256;            // threads per workgroup
constexpr int kActLutMaxBlocks = 2048;       // 256 CUs x 8 workgroups: a workgroup strides over the rest of the chunks
constexpr long kActLutMaxBytes = 0x7ffffffeL;    // 2^31 - 2: 32-bit byte offsets, as the other int8 NHWC entry points

struct ActLutGeom {
    unsigned n;                              // bytes of x and of y
    unsigned chunks, tail;                   // n / 16, n % 16
    unsigned C, Cpad;
    unsigned aligned;                        // Cpad % 16 == 0: a chunk lies inside one pixel and starts at a channel that is a multiple of 16
    unsigned blocks, passes;                 // workgroups; passes of the chunk loop (the same for every workgroup)
};

// status of the scalar arguments: 0 fine, -1 invalid, -4 over the index range (FQ_ERR_INVALID_ARG / FQ_ERR_UNSUPPORTED)
FQ_ACT_HD int act_lut_args(int N, int H, int W, int C, int Cpad) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || Cpad < C) return -1;
    long n = (long)N * H;
    if (n > kActLutMaxBytes) return -4;
    n *= W;
    if (n > kActLutMaxBytes) return -4;
    n *= Cpad;
    return n > kActLutMaxBytes ? -4 : 0;
}

FQ_ACT_HD ActLutGeom act_lut_geom(unsigned npix, int C, int Cpad) {
    ActLutGeom g;
    g.n = npix * (unsigned)Cpad;
    g.chunks = g.n / 16u;
    g.tail = g.n % 16u;
    g.C = (unsigned)C; g.Cpad = (unsigned)Cpad;
    g.aligned = Cpad % 16 == 0;
    unsigned b = (g.chunks + (unsigned)kActLutBlock - 1u) / (unsigned)kActLutBlock;
    if (b < 1u) b = 1u;                                      // (a tensor below 16 bytes is all tail)
    g.blocks = b > (unsigned)kActLutMaxBlocks ? (unsigned)kActLutMaxBlocks : b;
    const unsigned stride = g.blocks * (unsigned)kActLutBlock;
    g.passes = (g.chunks + stride - 1u) / stride;
    return g;
}

// chunk of lane `tid` of workgroup `block` in pass p (64-bit: the last pass of a large tensor runs past 2^32 / 16 only in theory,
// but the comparison with g.chunks must not wrap)
FQ_ACT_HD unsigned long long act_lut_chunk(const ActLutGeom& g, unsigned block, unsigned tid, unsigned p) {
    return (unsigned long long)p * g.blocks * (unsigned)kActLutBlock + (unsigned long long)block * (unsigned)kActLutBlock + tid;
}

// bit k set: byte k of the 16 bytes at byte offset o is a real channel (c < C), clear: a padding channel, written as zero
FQ_ACT_HD unsigned act_lut_real_mask(const ActLutGeom& g, unsigned o) {
    if (g.C == g.Cpad) return 0xffffu;
    unsigned c = o % g.Cpad;
    if (g.aligned) {
        const unsigned real = c < g.C ? g.C - c : 0u;
        return real >= 16u ? 0xffffu : (1u << real) - 1u;
    }
    unsigned m = 0u;
    for (unsigned k = 0; k < 16u; ++k) {
        if (c < g.C) m |= 1u << k;
        if (++c == g.Cpad) c = 0u;
    }
    return m;
}

// four mask bits -> the byte mask of a dword
FQ_ACT_HD unsigned act_lut_byte_mask(unsigned bits4) {
    return ((bits4 & 1u) * 0xffu) | (((bits4 >> 1) & 1u) * 0xff00u) | (((bits4 >> 2) & 1u) * 0xff0000u) | (((bits4 >> 3) & 1u) * 0xff000000u);
}

// tail byte t (0 <= t < g.tail): its byte offset, and whether it is a real channel
FQ_ACT_HD unsigned act_lut_tail_offset(const ActLutGeom& g, unsigned t) { return g.chunks * 16u + t; }
FQ_ACT_HD bool act_lut_tail_real(const ActLutGeom& g, unsigned t) { return act_lut_tail_offset(g, t) % g.Cpad < g.C; }

}  // namespace fq
