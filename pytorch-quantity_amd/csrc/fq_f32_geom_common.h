// fq_f32_geom_common.h -- what the geometry headers of the strip-per-lane fp32 convolutions (fq_dwconv_f32_geom.h,
// fq_gconv_f32_geom.h) share: the host / device qualifier, the 1 x 4 output strip, the workgroup -> first tile map and the
// reciprocal division.  Like those headers it compiles as plain host C++ for the walkers under scripts/.
#pragma once

#if defined(__HIPCC__)
#define FQ_GEOM_HD __host__ __device__ __forceinline__
#else
#define FQ_GEOM_HD inline
#endif

namespace fq {

constexpr int kGeomStrip = 4;              // output columns per lane: one 16-byte store

// input columns a strip reads: (4 - 1) * stride + R, rounded up to whole 16-byte LDS reads
FQ_GEOM_HD int geom_strip_reads(int R, int stride) { return ((kGeomStrip - 1) * stride + R + 3) / 4; }

// Workgroup b of G runs on XCD b % 8, each with its own L2: an XCD takes a contiguous run of tiles, so the tiles that share
// input (row bands with their halo rows, a group's channel chunks) meet in one L2.  Then every workgroup steps by G.
FQ_GEOM_HD unsigned geom_first_tile(unsigned b, unsigned G) {
    const unsigned G8 = G & ~7u;
    return b < G8 ? (b & 7u) * (G8 >> 3) + (b >> 3) : b;
}

// e / d = geom_mulhi(e, ceil(2^32 / d)) for e * d < 2^32
FQ_GEOM_HD unsigned geom_mulhi(unsigned a, unsigned m) { return (unsigned)(((unsigned long long)a * m) >> 32); }

}  // namespace fq
