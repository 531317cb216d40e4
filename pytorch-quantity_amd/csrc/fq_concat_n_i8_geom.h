// fq_concat_n_i8_geom.h -- the lane -> (sources, offsets, masks, loads) arithmetic of the N-source int8 NHWC concatenation
// (fq_concat_n_i8.hip), kept apart from the kernel so that the same functions compile as host code:
// scripts/concat_n_geom_check.cpp walks them over the shapes the GPU tests run.
//
// Chunks, lanes and the launch are those of the two-source kernel (fq_concat_i8_geom.h, whose CatPart, cat_dword_mask,
// cat_src_pix_lu and launch constants are used as they are); what changes is that source i owns the output channels
// [base_i, base_i + C_i) with base_i = C_0 + ... + C_{i-1}, for up to kCatNMaxSrc sources, so one 16-byte chunk may hold bytes
// of every one of them.
#pragma once

#include "fq_concat_i8_geom.h"

namespace fq {

constexpr int kCatNMaxSrc = 8;

struct CatNSrcGeom {
    int C, Cpad;                       // real / stored channels of the source
    int lu;                            // log2 of the nearest-upsampling factor (0, 1, 2), alike on both axes
    int base;                          // first output channel of the source
};

struct CatNGeom {
    int nsrc;
    CatNSrcGeom s[kCatNMaxSrc];        // entries at and behind nsrc: C = 0 (nothing of them lies in any chunk)
    int N, H, W;                       // OUTPUT plane; source i is [N][H >> lu][W >> lu][Cpad]
    int Cpad_out, CH;                  // CH = Cpad_out / 16
    unsigned npix;                     // N * H * W
};

// What source i contributes to the chunk k of every pixel (the fields of fq_concat_i8_geom.h's CatPart).
FQ_CAT_HD CatPart catn_part(const CatNGeom& g, int k, int i) {
    CatPart p;
    const int C = g.s[i].C;
    p.s = 16 * k - g.s[i].base;
    p.lo = p.s < 0 ? -p.s : 0;
    p.hi = C - p.s < 16 ? C - p.s : 16;
    p.use = i < g.nsrc && p.lo < p.hi;
    p.a = p.s & ~3;
    p.sh = p.s & 3;
    p.ld = 0u;
    p.whole16 = 0;
    if (!p.use) return p;
    for (int t = 0; t < 5; ++t) {
        const int o = p.a + 4 * t;                          // wanted bytes of the row: [s + lo, s + hi), inside [0, C)
        if (o < p.s + p.hi && o + 4 > p.s + p.lo) p.ld |= 1u << t;
    }
    p.whole16 = p.lo == 0 && (p.s & 15) == 0;
    return p;
}

// every base_i % 16 == 0: each chunk is 16 bytes of exactly one source at a 16-byte-aligned offset (the aligned family)
FQ_CAT_HD bool catn_aligned(const CatNGeom& g) {
    bool a = true;
    for (int i = 0; i < kCatNMaxSrc; ++i) a = a && (i >= g.nsrc || (g.s[i].base & 15) == 0);
    return a;
}

// number of sources with a byte in chunk k
FQ_CAT_HD int catn_owners(const CatNGeom& g, int k) {
    int n = 0;
    for (int i = 0; i < kCatNMaxSrc; ++i) n += catn_part(g, k, i).use;
    return n;
}

// The chunk is one 16-byte load of source i: nobody else has a byte in it and it starts on a 16-byte boundary of the source's
// row (hi < 16 only behind the last source: the tail mask).  Both families take this path for such a chunk.
FQ_CAT_HD bool catn_one16(const CatNGeom& g, int k, int i) {
    const CatPart p = catn_part(g, k, i);
    return p.use && p.whole16 && catn_owners(g, k) == 1;
}

// How the lanes that own chunk k build it, in the classes of fq_concat_i8_geom.h: kCatAligned16 one 16-byte load, kCatDword
// aligned dwords of one source, kCatByte byte-shifted dwords of one source, kCatStraddle bytes of two or more sources.
FQ_CAT_HD int catn_chunk_class(const CatNGeom& g, int k) {
    if (catn_owners(g, k) > 1) return kCatStraddle;
    for (int i = 0; i < kCatNMaxSrc; ++i) {
        const CatPart p = catn_part(g, k, i);
        if (p.use) return p.whole16 ? kCatAligned16 : (p.sh == 0 ? kCatDword : kCatByte);
    }
    return kCatAligned16;                                   // (not reached: Cpad_out == pad16(sum C), every chunk has an owner)
}

// pixel index of a source upsampled by 2^lu under the output pixel (n, h, w)
FQ_CAT_HD unsigned catn_src_pix(const CatNGeom& g, int lu, unsigned n, unsigned h, unsigned w) {
    return (n * ((unsigned)g.H >> lu) + (h >> lu)) * ((unsigned)g.W >> lu) + (w >> lu);
}

// The launch is the two-source kernel's: lane gid owns chunk gid % CH of the pixels gid / CH, + stride, ... (cat_blocks).
FQ_CAT_HD long catn_blocks(const CatNGeom& g) {
    long b = ((long)g.npix * g.CH + kCatBlock - 1) / kCatBlock;
    return b > kCatMaxBlocks ? kCatMaxBlocks : b;
}

}  // namespace fq
