// Host check of the depthwise fp32 kernel's address arithmetic (csrc/fq_dwconv_f32_geom.h): over the GPU tests' shapes and the
// thirteen depthwise layers of model/mobilenet/MobileNet_fabu.py at N = 1, every lane of every launch (the plain grid and the
// histogram form's smaller one) loads inside x, indexes LDS inside the staged tile, stores inside y, and every output element is
// written exactly once.  It also checks that the LDS float a lane reads for a tap is the one the staging filled from that tap's
// pixel (or with zero, where the pixel lies outside the image), and the reciprocal-multiply divisions against real ones.
//   c++ -O2 -std=c++17 -o dwconv_f32_geom_check scripts/dwconv_f32_geom_check.cpp && ./dwconv_f32_geom_check
//   ./dwconv_f32_geom_check window=T N,C,H,W,R,stride,pad     a size-limit row instead of the lists: every workgroup of the plain
//                                  grid, but only the first and the last T tiles.  A top row's output is 4.29 GB and does cross 2^31
//                                  bytes in between; the tiles there are not walked, because nothing in this kernel is a byte offset:
//                                  it indexes plain pointers with UNSIGNED 32-bit ELEMENT offsets, below 2^30 by the host's guard, so
//                                  bit 31 of a byte address is never a bit of a 32-bit quantity.  Every such offset of the walked
//                                  tiles is checked against 64-bit arithmetic, and the tile index must not wrap
// (tests/test_depthwise_f32_cpu.py runs it.)  The walk below is the kernel's own: same plan, same grid, same workgroup -> tiles,
// same lane -> strip, the same predicates in front of every access.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_dwconv_f32_geom.h"

using namespace fq;

struct Shape { int N, C, H, W, R, stride, pad; };

static void fail(const char* what, const Shape& s) {
    printf("%s: N %d, C %d, H %d, W %d, %dx%d stride %d, pad %d\n", what, s.N, s.C, s.H, s.W, s.R, s.R, s.stride, s.pad);
    exit(1);
}

static unsigned long g_window = 0;          // window=T: tiles [T, tiles - T) are skipped

static long run(const Shape& s, bool hist) {
    DwfGeom g;
    if (!dwf_plan(g, s.N, s.C, s.H, s.W, s.R, s.stride, s.pad)) fail("the plan declines a shape of the list", s);
    const int R = s.R, nrd = geom_strip_reads(R, s.stride);
    const size_t in_elems = (size_t)s.N * s.C * s.H * s.W, out_elems = (size_t)s.N * s.C * g.Ho * g.Wo;
    if (g.fill > (unsigned)kDwfLdsFloats || g.PP > kDwfMaxPP || g.PP < 1 || g.TH * g.QW * g.PP > kDwfBlock || (g.IWP & 3))
        fail("tile larger than the workgroup or its LDS", s);
    const bool windowed = g_window && (unsigned long)g.tiles > 2 * g_window;
    // a windowed walk keeps the outputs of the first and the last `keep` elements only: whole plane groups of the two windows
    const size_t per_grp = (size_t)g.RB * g.CB, grps = (g.planes + g.PP - 1) / g.PP, kgrp = windowed ? g_window / per_grp : 0;
    const size_t plane_out = (size_t)g.Ho * g.Wo, keep = windowed ? (kgrp + 1) * g.PP * plane_out : out_elems;
    if (windowed && (kgrp < 1 || 2 * keep > out_elems)) fail("window smaller than one plane group, or as large as the tensor", s);
    if (in_elems * 4 > 0xffffffffUL || out_elems * 4 > 0xffffffffUL || (unsigned long)g.tiles + kDwfMaxBlocks > 0xffffffffUL ||
        (unsigned long)grps * per_grp != g.tiles)
        fail("32-bit tile or offset arithmetic wraps", s);
    auto slot = [&](size_t o) -> size_t {
        if (!windowed) return o;
        if (o < keep) return o;
        if (o >= out_elems - keep) return keep + (o - (out_elems - keep));
        fail("a tile of a window stores into the middle of the tensor", s);
        return 0;
    };
    std::vector<unsigned char> written(windowed ? 2 * keep : out_elems, 0);
    std::vector<long> src(g.fill);                        // what the staging left in each LDS float: element offset, or -1 for zero
    const unsigned G = dwf_grid(g, hist);
    long loads = 0;
    for (unsigned b = 0; b < G; ++b) {
        for (unsigned tile = geom_first_tile(b, G); tile < g.tiles; tile += G) {
            if (windowed && tile >= g_window && tile < g.tiles - g_window) {   // jump to this workgroup's first tile of the last window
                const unsigned long steps = ((unsigned long)(g.tiles - g_window) - tile + G - 1) / G;
                const unsigned long next = tile + steps * G;
                if (next >= g.tiles) break;
                tile = (unsigned)(next - G);
                continue;
            }
            const DwfTilePos tp = dwf_tile_pos(g, tile);
            if (tp.plane0 >= g.planes || tp.oh0 >= g.Ho || tp.ow0 >= g.Wo) fail("tile outside the tensor", s);
            for (unsigned e = 0; e < g.fill; ++e) {       // (lane e % 256 in step e / 256: every e < fill exactly once)
                unsigned off = 0;
                const bool ld = dwf_fill_src(g, tp, e, &off);
                const unsigned pi = e / g.slot, rem = e % g.slot, r = rem / g.IWP, col = rem % g.IWP;
                if (geom_mulhi(e, g.m_slot) != pi || geom_mulhi(rem, g.m_pitch) != r) fail("reciprocal division is off", s);
                const long ih = (long)tp.oh0 * s.stride - s.pad + r, iw = (long)tp.ow0 * s.stride - s.pad + col;
                const bool want = tp.plane0 + pi < g.planes && ih >= 0 && ih < s.H && iw >= 0 && iw < s.W;
                if (ld != want) fail("staging predicate is off", s);
                if (ld) {
                    if ((size_t)off >= in_elems) fail("load outside the input", s);
                    if ((long)off != ((long)(tp.plane0 + pi) * s.H + ih) * s.W + iw) fail("load of the wrong pixel", s);
                    ++loads;
                }
                src[e] = ld ? (long)off : -1;
            }
            for (unsigned tid = 0; tid < (unsigned)kDwfBlock; ++tid) {
                const DwfLanePos lp = dwf_lane_pos(g, tid);
                const int cnt = dwf_out_count(g, tp, lp);
                if (cnt == 0) continue;
                const unsigned rd0 = dwf_read_index(g, lp), o = dwf_out_off(g, tp, lp);
                if (rd0 & 3u) fail("LDS read not 16-byte aligned", s);
                const long plane = (long)tp.plane0 + lp.pi, oh = tp.oh0 + lp.t, ow = tp.ow0 + lp.q * kDwfStrip;
                for (int r = 0; r < R; ++r) {
                    if ((size_t)rd0 + (size_t)r * g.IWP + 4u * nrd > g.fill) fail("LDS index outside the staged tile", s);
                    for (int j = 0; j < cnt; ++j)
                        for (int t = 0; t < R; ++t) {
                            const long ih = oh * s.stride - s.pad + r, iw = (ow + j) * s.stride - s.pad + t;
                            const bool in = ih >= 0 && ih < s.H && iw >= 0 && iw < s.W;
                            const long want = in ? (plane * s.H + ih) * s.W + iw : -1;
                            if (src[rd0 + r * g.IWP + j * s.stride + t] != want) fail("a tap reads another pixel's LDS float", s);
                        }
                }
                for (int j = 0; j < cnt; ++j) {
                    if ((size_t)o + j >= out_elems) fail("store outside the output", s);
                    if ((long)o + j != (plane * g.Ho + oh) * g.Wo + ow + j) fail("store to the wrong element", s);
                    if (written[slot((size_t)o + j)]++) fail("output element written twice", s);
                }
            }
        }
    }
    if (!windowed) {
        for (unsigned char v : written)
            if (v != 1) fail("output element not written", s);
    } else {                                              // the planes of the whole groups that the two windows cover
        const size_t head = kgrp * g.PP * plane_out, tail0 = (grps - kgrp) * g.PP * plane_out;
        for (size_t o = 0; o < head; ++o)
            if (written[slot(o)] != 1) fail("output element of the first planes not written", s);
        for (size_t o = tail0; o < out_elems; ++o)
            if (written[slot(o)] != 1) fail("output element of the last planes not written", s);
    }
    return loads;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        long total = 0;
        for (int a = 1; a < argc; ++a) {
            Shape s;
            if (strncmp(argv[a], "window=", 7) == 0) { g_window = strtoul(argv[a] + 7, nullptr, 10); continue; }
            if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d", &s.N, &s.C, &s.H, &s.W, &s.R, &s.stride, &s.pad) != 7) {
                printf("cannot read case %s\n", argv[a]);
                return 2;
            }
            total += run(s, false);
        }
        printf("ok, %ld loads\n", total);
        return 0;
    }
    // tests/test_gpu_depthwise_f32.py: SHAPES
    const Shape tests[] = {{1, 1, 1, 1, 3, 1, 1},   {2, 3, 3, 3, 3, 1, 0},    {1, 5, 4, 6, 5, 1, 4},   {3, 7, 7, 7, 3, 1, 1},
                           {2, 19, 14, 14, 3, 2, 1}, {2, 4, 13, 9, 5, 2, 2},   {1, 3, 17, 23, 3, 2, 0}, {1, 2, 56, 56, 3, 1, 1},
                           {1, 2, 112, 112, 3, 2, 1}, {1, 1, 5, 300, 3, 1, 1}, {1, 1, 300, 5, 5, 1, 2}, {2, 67, 7, 7, 5, 1, 2},
                           {64, 32, 7, 7, 3, 1, 1}};
    // the depthwise layers of MobileNet_fabu at 224 x 224 (both variants: the residual one has 5x5 kernels in the last stage)
    const Shape net[] = {{1, 32, 112, 112, 3, 1, 1}, {1, 64, 112, 112, 3, 2, 1}, {1, 128, 56, 56, 3, 1, 1}, {1, 128, 56, 56, 3, 2, 1},
                         {1, 256, 28, 28, 3, 1, 1},  {1, 256, 28, 28, 3, 2, 1},  {1, 512, 14, 14, 3, 1, 1}, {1, 512, 14, 14, 3, 1, 1},
                         {1, 512, 14, 14, 3, 1, 1},  {1, 512, 14, 14, 3, 1, 1},  {1, 512, 14, 14, 3, 1, 1}, {1, 512, 14, 14, 3, 2, 1},
                         {1, 1024, 7, 7, 3, 1, 1},   {1, 512, 14, 14, 5, 2, 2},  {1, 1024, 7, 7, 5, 1, 2}};
    long total = 0;
    for (const Shape& s : tests)
        for (bool hist : {false, true}) total += run(s, hist);
    for (const Shape& s : net)
        for (bool hist : {false, true}) total += run(s, hist);
    // more tiles than either grid has workgroups, with a partly filled last plane group; every padding of both kernels at an odd size
    total += run({300, 131, 7, 7, 3, 1, 1}, false);
    total += run({5, 40, 56, 56, 3, 1, 1}, true);
    for (int R : {3, 5})
        for (int stride : {1, 2})
            for (int pad = 0; pad < R; ++pad)
                for (bool hist : {false, true}) total += run({2, 5, 9, 11, R, stride, pad}, hist);
    printf("ok, %ld loads\n", total);
    return 0;
}
