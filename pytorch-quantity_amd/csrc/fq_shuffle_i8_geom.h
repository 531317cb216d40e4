// fq_shuffle_i8_geom.h -- the index arithmetic of the int8 NHWC channel shuffle / channel slice (fq_shuffle_i8.hip), kept apart
// from the kernel so that the same functions compile as host code: scripts/shuffle_geom_check.cpp walks them over the shapes the
// GPU tests run and asserts that every address a lane touches lies inside its tensor, that every output byte is written exactly
// once and that it comes from the channel the rule names.
//
//   y[pix][j] = x[pix][c_off + (j % g) * (C / g) + j / g]     0 <= j < C          (g == 1: the slice [c_off, c_off + C))
//             = 0                                             C <= j < Cpad_out
//
// The source row is [Cpad_in] bytes, the output row [Cpad_out] bytes, CH = Cpad_out / 16 UNITS (one dwordx4 store each).  Of a
// source row only the aligned SPAN [a0, a0 + S) is read: a0 = c_off rounded down to 16, a0 + S = c_off + C rounded up to 16, which
// is <= Cpad_in because Cpad_in % 16 == 0.  A TILE is TP consecutive pixels; a workgroup stages the spans of a tile's pixels in
// LDS with 16-byte loads (stage item i = pixel i / (S / 16), 16-byte piece i % (S / 16), at LDS byte 16 i: linear in the lane),
// then every lane puts output units together from LDS bytes and stores them.  A span that does not fit the LDS budget even for
// one pixel (C above about 32 K) is read from global memory byte by byte instead (lds == 0, TP = kShufTilePix).
#pragma once

#if defined(__HIPCC__)
#define FQ_SHUF_HD __host__ __device__ __forceinline__
#else
#define FQ_SHUF_HD inline
#endif

namespace fq {

constexpr int kShufBlock = 256;            // threads per workgroup
constexpr int kShufMaxBlocks = 2048;       // 256 CUs x 8 workgroups: a workgroup strides over the rest of the tiles
constexpr int kShufTilePix = 64;           // pixels per tile where the spans fit
constexpr int kShufLdsBytes = 32768;       // LDS of one workgroup (five of them fit a CU's 160 KiB)
constexpr int kShufMaxC = 65536;

struct ShufGeom {
    int Cpad_in, c_off, C, g, cg;          // cg = C / g
    int Cpad_out, CH;                      // CH = Cpad_out / 16
    int a0, S, SU;                         // span [a0, a0 + S) of a source row; SU = S / 16
    int lds;                               // 1: spans staged in LDS
    int TP;                                // pixels per tile
    unsigned npix, ntiles;
};

FQ_SHUF_HD int shuf_pad16(int c) { return (c + 15) / 16 * 16; }

// the scalar preconditions of the rule (no pointer, no plane)
FQ_SHUF_HD bool shuf_args_ok(int Cpad_in, int c_off, int C, int g) {
    return C >= 1 && c_off >= 0 && g >= 1 && C % g == 0 && Cpad_in >= 16 && Cpad_in % 16 == 0 && (long)c_off + C <= Cpad_in
        && C <= kShufMaxC;
}

FQ_SHUF_HD ShufGeom shuf_geom(int Cpad_in, int c_off, int C, int g, unsigned npix) {
    ShufGeom s;
    s.Cpad_in = Cpad_in; s.c_off = c_off; s.C = C; s.g = g; s.cg = C / g;
    s.Cpad_out = shuf_pad16(C); s.CH = s.Cpad_out / 16;
    s.a0 = c_off & ~15;
    s.S = shuf_pad16(c_off + C) - s.a0;
    s.SU = s.S / 16;
    s.lds = s.S <= kShufLdsBytes;
    const int fit = s.lds ? kShufLdsBytes / s.S : kShufTilePix;
    s.TP = fit < kShufTilePix ? fit : kShufTilePix;
    s.npix = npix;
    s.ntiles = (npix + (unsigned)s.TP - 1u) / (unsigned)s.TP;
    return s;
}

FQ_SHUF_HD unsigned shuf_blocks(const ShufGeom& s) { return s.ntiles > (unsigned)kShufMaxBlocks ? (unsigned)kShufMaxBlocks : s.ntiles; }

// pixels of tile t (the last one may be short)
FQ_SHUF_HD unsigned shuf_tile_pixels(const ShufGeom& s, unsigned t) {
    const unsigned left = s.npix - t * (unsigned)s.TP;
    return left < (unsigned)s.TP ? left : (unsigned)s.TP;
}

// stage item i of a tile whose first pixel is pix0: 16 bytes from this byte offset of x go to LDS byte 16 * i
FQ_SHUF_HD size_t shuf_stage_src(const ShufGeom& s, unsigned pix0, unsigned i) {
    const unsigned p = i / (unsigned)s.SU, u = i - p * (unsigned)s.SU;
    return (size_t)(pix0 + p) * (size_t)s.Cpad_in + (size_t)s.a0 + 16u * (size_t)u;
}

// where pixel p (of the tile) keeps its channel c_off: LDS byte with `lds`, else the byte offset in x of pixel pix0 + p
FQ_SHUF_HD size_t shuf_row_base(const ShufGeom& s, unsigned pix0, unsigned p) {
    return s.lds ? (size_t)p * (size_t)s.S + (size_t)(s.c_off - s.a0) : (size_t)(pix0 + p) * (size_t)s.Cpad_in + (size_t)s.c_off;
}

// The walk over the 16 bytes of output unit k: output channel j = 16 k + b reads the row at rel = (j % g) * cg + j / g.  One
// division per unit, then increments.
struct ShufWalk {
    unsigned j, r, q;
};
FQ_SHUF_HD ShufWalk shuf_walk_begin(const ShufGeom& s, unsigned k) {
    ShufWalk w;
    w.j = 16u * k;
    w.q = w.j / (unsigned)s.g;
    w.r = w.j - w.q * (unsigned)s.g;
    return w;
}
FQ_SHUF_HD bool shuf_walk_real(const ShufGeom& s, const ShufWalk& w) { return w.j < (unsigned)s.C; }
FQ_SHUF_HD unsigned shuf_walk_rel(const ShufGeom& s, const ShufWalk& w) { return w.r * (unsigned)s.cg + w.q; }
FQ_SHUF_HD void shuf_walk_next(const ShufGeom& s, ShufWalk& w) {
    ++w.j;
    if (++w.r == (unsigned)s.g) { w.r = 0u; ++w.q; }
}

}  // namespace fq
