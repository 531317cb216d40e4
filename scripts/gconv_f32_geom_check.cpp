// Host check of the grouped fp32 kernel's address arithmetic (csrc/fq_gconv_f32_geom.h): over the GPU tests' shapes and the
// sixteen grouped 3x3 layers of model/resnext/ResNeXt_fabu.py (ResNeXt50) at N = 1, every lane of every launch (the plain grid
// and the histogram form's smaller one) loads inside x and w, indexes LDS inside the staged tile, stores inside y, and every
// output element is written exactly once.  It also checks that the LDS float a lane reads for a tap is the one the staging
// filled from that tap's pixel and channel (or with zero, where the pixel lies outside the image), that the LDS weight it reads
// for (k, c, r, s) was staged from that weight, and the reciprocal-multiply divisions against real ones.
//   c++ -O2 -std=c++17 -o gconv_f32_geom_check scripts/gconv_f32_geom_check.cpp && ./gconv_f32_geom_check
// (tests/test_grouped_f32_cpu.py runs it.)  The walk below is the kernel's own: same plan, same grid, same workgroup -> tiles,
// same lane -> strip, the same predicates in front of every access.
//   ./gconv_f32_geom_check window=T N,G,Cgi,Cgo,H,W,R,stride,pad    a size-limit row instead of the lists: every workgroup of the
//                                  plain grid, but only the first and the last T tiles.  A top row's output is 4.29 GB and does cross
//                                  2^31 bytes in between; the tiles there are not walked, because nothing in this kernel is a byte
//                                  offset: it indexes plain pointers with UNSIGNED 32-bit ELEMENT offsets, below 2^30 by the host's
//                                  guard.  Every such offset of the walked tiles is checked against 64-bit arithmetic, and the tile
//                                  index must not wrap
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_gconv_f32_geom.h"

using namespace fq;

struct Shape { int N, G, Cgi, Cgo, H, W, R, stride, pad; };

static void fail(const char* what, const Shape& s) {
    printf("%s: N %d, groups %d, %d -> %d per group, H %d, W %d, %dx%d stride %d, pad %d\n", what, s.N, s.G, s.Cgi, s.Cgo, s.H, s.W,
           s.R, s.R, s.stride, s.pad);
    exit(1);
}

static unsigned long g_window = 0;          // window=T: tiles [T, tiles - T) are skipped

static long run(const Shape& s, bool hist) {
    GfGeom g;
    const int C = s.G * s.Cgi, K = s.G * s.Cgo, R = s.R, RR = R * R;
    if (!gf_plan(g, s.N, C, s.H, s.W, K, s.G, R, s.stride, s.pad)) fail("the plan declines a shape of the list", s);
    const int nrd = geom_strip_reads(R, s.stride);
    const size_t in_elems = (size_t)s.N * C * s.H * s.W, out_elems = (size_t)s.N * K * g.Ho * g.Wo;
    const size_t w_elems = (size_t)K * s.Cgi * RR;
    if (g.fill > g.in_floats || g.in_floats < (unsigned)kGfMinInFloats || g.b0 != g.wfill || g.x0 < g.b0 + (unsigned)g.KC || (g.x0 & 3u) ||
        g.x0 + g.in_floats > (unsigned)kGfLdsFloats || g.wfill > (unsigned)kGfWFloats || g.KC > kGfMaxKC || (g.KC & 3) || g.KC < 4 ||
        g.KBN * g.TH * g.QW > kGfBlock || g.TH < 1 || g.QW < 1 || (g.IWP & 3) || g.KC * g.KCN < s.Cgo || g.TH * g.RB < g.Ho ||
        g.QW * g.CB * kGfStrip < g.Wo)
        fail("tile larger than the workgroup or its LDS, or the tiles do not cover the layer", s);
    const bool windowed = g_window && (unsigned long)g.tiles > 2 * g_window;
    // a windowed walk keeps the outputs of the first and the last `keep` elements only: whole (image, group) units of the two windows
    const size_t per_unit = (size_t)g.KCN * g.RB * g.CB, kunit = windowed ? g_window / per_unit : 0;
    const size_t unit_out = (size_t)s.Cgo * g.Ho * g.Wo, keep = windowed ? (kunit + 1) * unit_out : out_elems;
    if (windowed && (kunit < 1 || 2 * keep > out_elems)) fail("window smaller than one (image, group) unit, or as large as the tensor", s);
    if (in_elems * 4 > 0xffffffffUL || out_elems * 4 > 0xffffffffUL || w_elems * 4 > 0xffffffffUL ||
        (unsigned long)g.tiles + kGfMaxBlocks > 0xffffffffUL || (unsigned long)g.units * per_unit != g.tiles)
        fail("32-bit tile or offset arithmetic wraps", s);
    auto slot = [&](size_t o) -> size_t {
        if (!windowed || o < keep) return o;
        if (o >= out_elems - keep) return keep + (o - (out_elems - keep));
        fail("a tile of a window stores into the middle of the tensor", s);
        return 0;
    };
    std::vector<unsigned char> written(windowed ? 2 * keep : out_elems, 0);
    std::vector<long> src(g.fill);                        // what the staging left in each LDS float: element offset, or -1 for zero
    std::vector<long> wsrc(g.wfill);                      // the same for the weight block; -2: not staged
    const unsigned G = gf_grid(g, hist);
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
            const GfTilePos tp = gf_tile_pos(g, tile);
            if (tp.n >= (unsigned)s.N || tp.grp >= (unsigned)s.G || tp.k0 >= s.Cgo || tp.oh0 >= g.Ho || tp.ow0 >= g.Wo)
                fail("tile outside the tensor", s);
            for (unsigned e = 0; e < g.fill; ++e) {       // (lane e % 256 in step e / 256: every e < fill exactly once)
                unsigned off = 0;
                const bool ld = gf_fill_src(g, tp, e, &off);
                const unsigned c = e / g.slot, rem = e % g.slot, r = rem / g.IWP, col = rem % g.IWP;
                if (geom_mulhi(e, g.m_slot) != c || geom_mulhi(rem, g.m_pitch) != r) fail("reciprocal division is off", s);
                const long ih = (long)tp.oh0 * s.stride - s.pad + r, iw = (long)tp.ow0 * s.stride - s.pad + col;
                const bool want = ih >= 0 && ih < s.H && iw >= 0 && iw < s.W;
                if (ld != want) fail("staging predicate is off", s);
                if (ld) {
                    if ((size_t)off >= in_elems) fail("load outside the input", s);
                    if ((long)off != (((long)tp.n * C + (long)tp.grp * s.Cgi + c) * s.H + ih) * s.W + iw) fail("load of the wrong pixel", s);
                    ++loads;
                }
                src[e] = ld ? (long)off : -1;
            }
            for (long& v : wsrc) v = -2;
            for (unsigned i = 0; i < g.wfill; ++i) {
                unsigned off = 0, dst = 0;
                const bool ld = gf_w_src(g, tp, i, &off, &dst);
                const unsigned kk = i / g.ckr, rem = i % g.ckr, c = rem / RR, tap = rem % RR;
                if (geom_mulhi(i, g.m_ckr) != kk || (RR != 1 && geom_mulhi(rem, g.m_rr) != c)) fail("reciprocal division is off (weights)", s);
                if (dst >= g.wfill) fail("LDS weight index outside the staged block", s);
                if (dst != (tap * s.Cgi + c) * g.KC + kk) fail("weight staged to the wrong LDS float", s);
                if (wsrc[dst] != -2) fail("LDS weight float staged twice", s);
                if (ld != (tp.k0 + (int)kk < s.Cgo)) fail("weight staging predicate is off", s);
                if (ld) {
                    if ((size_t)off >= w_elems) fail("load outside the weights", s);
                    if ((long)off != (((long)tp.grp * s.Cgo + tp.k0 + kk) * s.Cgi + c) * RR + tap) fail("load of the wrong weight", s);
                    ++loads;
                }
                wsrc[dst] = ld ? (long)off : -1;
            }
            for (unsigned tid = 0; tid < (unsigned)kGfBlock; ++tid) {
                const GfLanePos lp = gf_lane_pos(g, tid);
                const int cnt = gf_out_count(g, tp, lp);
                if (cnt == 0) continue;
                if (lp.kb >= g.KBN || lp.t >= g.TH || lp.q >= g.QW) fail("lane outside the tile", s);
                const unsigned rd0 = gf_read_index(g, lp);
                if (rd0 & 3u) fail("LDS read not 16-byte aligned", s);
                const long oh = tp.oh0 + lp.t, ow = tp.ow0 + lp.q * kGfStrip;
                for (int c = 0; c < s.Cgi; ++c)
                    for (int r = 0; r < R; ++r) {
                        const size_t row = (size_t)rd0 + (size_t)c * g.slot + (size_t)r * g.IWP;
                        if (row + 4u * nrd > g.fill) fail("LDS index outside the staged tile", s);
                        const long plane = (long)tp.n * C + (long)tp.grp * s.Cgi + c;
                        for (int j = 0; j < cnt; ++j)
                            for (int t = 0; t < R; ++t) {
                                const long ih = oh * s.stride - s.pad + r, iw = (ow + j) * s.stride - s.pad + t;
                                const bool in = ih >= 0 && ih < s.H && iw >= 0 && iw < s.W;
                                const long want = in ? (plane * s.H + ih) * s.W + iw : -1;
                                if (src[row + j * s.stride + t] != want) fail("a tap reads another pixel's LDS float", s);
                            }
                        for (int t = 0; t < R; ++t) {
                            const unsigned wi = gf_w_index(g, lp, r * R + t, c);
                            if ((wi & 3u) || wi + kGfKB > g.wfill) fail("LDS weight read misaligned or outside the staged block", s);
                            for (int kk = 0; kk < kGfKB; ++kk) {
                                const long k = (long)tp.grp * s.Cgo + tp.k0 + lp.kb * kGfKB + kk;
                                if (wsrc[wi + kk] != (k * s.Cgi + c) * RR + r * R + t) fail("a tap reads another weight's LDS float", s);
                            }
                        }
                    }
                for (int kk = 0; kk < kGfKB; ++kk) {
                    const unsigned o = gf_out_off(g, tp, lp, kk);
                    const long kin = tp.k0 + lp.kb * kGfKB + kk;
                    if (kin >= s.Cgo || kin >= tp.k0 + g.KC) fail("output channel outside the group or the chunk", s);
                    const long plane = (long)tp.n * K + (long)tp.grp * s.Cgo + kin;
                    for (int j = 0; j < cnt; ++j) {
                        if ((size_t)o + j >= out_elems) fail("store outside the output", s);
                        if ((long)o + j != (plane * g.Ho + oh) * g.Wo + ow + j) fail("store to the wrong element", s);
                        if (written[slot((size_t)o + j)]++) fail("output element written twice", s);
                    }
                }
            }
        }
    }
    if (!windowed) {
        for (unsigned char v : written)
            if (v != 1) fail("output element not written", s);
    } else {                                              // the whole units that the two windows cover
        for (size_t o = 0; o < kunit * unit_out; ++o)
            if (written[slot(o)] != 1 || written[slot(out_elems - 1 - o)] != 1) fail("output element of the first or last units not written", s);
    }
    return loads;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        long walked = 0;
        for (int a = 1; a < argc; ++a) {
            Shape s;
            if (strncmp(argv[a], "window=", 7) == 0) { g_window = strtoul(argv[a] + 7, nullptr, 10); continue; }
            if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d,%d,%d", &s.N, &s.G, &s.Cgi, &s.Cgo, &s.H, &s.W, &s.R, &s.stride, &s.pad) != 9) {
                printf("cannot read case %s\n", argv[a]);
                return 2;
            }
            walked += run(s, false);
        }
        printf("ok, %ld loads\n", walked);
        return 0;
    }
    // tests/test_gpu_grouped_f32.py: SHAPES
    const Shape tests[] = {{1, 2, 4, 4, 1, 1, 1, 1, 0},   {1, 2, 4, 4, 1, 1, 3, 1, 1},    {2, 3, 4, 8, 3, 3, 3, 1, 0},   {1, 2, 8, 4, 5, 7, 3, 2, 1},
                           {3, 2, 12, 12, 7, 7, 3, 1, 1}, {1, 2, 4, 4, 6, 6, 3, 1, 2},    {2, 32, 4, 4, 14, 14, 3, 1, 1}, {2, 2, 32, 32, 7, 7, 3, 1, 1},
                           {1, 2, 64, 64, 6, 6, 3, 2, 1}, {1, 4, 20, 36, 5, 5, 1, 2, 0},  {2, 5, 4, 64, 4, 4, 1, 1, 0},  {1, 2, 16, 16, 9, 300, 3, 1, 1},
                           {1, 2, 16, 16, 300, 9, 3, 2, 1}, {33, 64, 4, 4, 7, 7, 3, 1, 1}, {1, 2, 64, 40, 3, 3, 3, 1, 1},
                           {1, 2, 4, 4, 3, 70, 3, 1, 1},  {1, 2, 64, 4, 24, 3, 3, 1, 1}};
    // the grouped 3x3 layers of ResNeXt50 (32 x 4d) at 224 x 224: the first block of stages 2 to 4 has stride 2
    const Shape net[] = {{1, 32, 4, 4, 56, 56, 3, 1, 1},  {1, 32, 4, 4, 56, 56, 3, 1, 1},  {1, 32, 4, 4, 56, 56, 3, 1, 1},
                         {1, 32, 8, 8, 56, 56, 3, 2, 1},  {1, 32, 8, 8, 28, 28, 3, 1, 1},  {1, 32, 8, 8, 28, 28, 3, 1, 1},
                         {1, 32, 8, 8, 28, 28, 3, 1, 1},  {1, 32, 16, 16, 28, 28, 3, 2, 1}, {1, 32, 16, 16, 14, 14, 3, 1, 1},
                         {1, 32, 16, 16, 14, 14, 3, 1, 1}, {1, 32, 16, 16, 14, 14, 3, 1, 1}, {1, 32, 16, 16, 14, 14, 3, 1, 1},
                         {1, 32, 16, 16, 14, 14, 3, 1, 1}, {1, 32, 32, 32, 14, 14, 3, 2, 1}, {1, 32, 32, 32, 7, 7, 3, 1, 1},
                         {1, 32, 32, 32, 7, 7, 3, 1, 1}};
    long total = 0;
    for (const Shape& s : tests)
        for (bool hist : {false, true}) total += run(s, hist);
    for (const Shape& s : net)
        for (bool hist : {false, true}) total += run(s, hist);
    // more tiles than either grid has workgroups; every padding of both kernels at an odd size, with unequal channel counts and
    // with a group whose output channels take more than one chunk
    total += run({40, 32, 4, 4, 28, 28, 3, 1, 1}, false);
    total += run({5, 32, 8, 8, 56, 56, 3, 1, 1}, true);
    for (int R : {1, 3})
        for (int stride : {1, 2})
            for (int pad = 0; pad < R; ++pad)
                for (bool hist : {false, true}) {
                    total += run({2, 3, 8, 12, 9, 11, R, stride, pad}, hist);
                    total += run({1, 2, 64, 40, 9, 11, R, stride, pad}, hist);
                }
    printf("ok, %ld loads\n", total);
    return 0;
}
