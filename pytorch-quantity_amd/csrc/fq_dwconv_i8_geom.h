// fq_dwconv_i8_geom.h -- the tile / lane -> address arithmetic of the depthwise int8 convolution (fq_dwconv_i8.hip), kept apart
// from the kernel so that the same functions compile as host code: scripts/dwconv_geom_check.cpp walks them over the shapes
// the GPU tests run and asserts that every address a lane may touch lies inside its tensor and every output dword is written once.
#pragma once

#if defined(__HIPCC__)
#define FQ_DW_HD __host__ __device__ __forceinline__
#else
#define FQ_DW_HD inline
#endif

namespace fq {

constexpr int kDwBlock = 256;          // threads per workgroup
constexpr int kDwTQ = 4;               // output columns per lane (one transposed dword = 4 pixels of one channel)
constexpr int kDwMaxBlocks = 2048;     // 256 CUs x 8 workgroups: the lanes walk the rest of the tiles

// output rows per lane: an input row is read once for every output row of the tile it serves, (TP - 1) * stride + R rows for TP
// outputs; 5x5 holds twice the weights in registers and takes the smaller tile
#ifndef FQ_DW_TP3
#define FQ_DW_TP3 4
#endif
#ifndef FQ_DW_TP5
#define FQ_DW_TP5 2
#endif
template <int R> struct DwTile { static constexpr int TP = R == 3 ? FQ_DW_TP3 : FQ_DW_TP5; };

struct DwGeom {
    int N, H, W, P, Q, Cpad, C4;       // C4 = Cpad / 4: one lane = 4 channels
    int pad_h, pad_w;
    int PB, QB;                        // tiles per image: row bands x column blocks
    unsigned tiles;                    // N * PB * QB
};

// lane g of the launch: channel group c4 = g % C4, first tile g / C4, every lane steps by sp_stride = threads / C4 tiles;
// lanes beyond C4 * sp_stride do nothing
struct DwTilePos { int n, p0, q0; };
template <int TP>
FQ_DW_HD DwTilePos dw_tile_pos(const DwGeom& g, unsigned tile) {
    DwTilePos t;
    const unsigned qb = tile % (unsigned)g.QB, rest = tile / (unsigned)g.QB;
    t.q0 = (int)qb * kDwTQ;
    t.p0 = (int)(rest % (unsigned)g.PB) * TP;
    t.n = (int)(rest / (unsigned)g.PB);
    return t;
}
// element offset of input pixel (n, ih, iw), channel group c4; valid only where dw_in_ok says so
FQ_DW_HD bool dw_in_ok(const DwGeom& g, int ih, int iw) { return (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W; }
FQ_DW_HD unsigned dw_in_off(const DwGeom& g, int n, int ih, int iw, int c4) {
    return (((unsigned)n * g.H + ih) * g.W + iw) * g.Cpad + 4u * c4;
}
FQ_DW_HD bool dw_out_ok(const DwGeom& g, int p, int q) { return p < g.P && q < g.Q; }
FQ_DW_HD unsigned dw_out_off(const DwGeom& g, int n, int p, int q, int c4) {
    return (((unsigned)n * g.P + p) * g.Q + q) * g.Cpad + 4u * c4;
}

}  // namespace fq
