// Host check of the atrous depthwise fp32 kernel's address arithmetic (csrc/fq_dwconv_dil_f32_geom.h): over the GPU tests' shapes
// and the atrous depthwise layers of model/deeplab/DeepLabV3Plus_fabu.py, every lane of every launch (the plain grid and the
// histogram form's smaller one) stages only elements from inside x, reads LDS only inside the staged rows or the zero row, and
// every output element is written exactly once.  It also checks that the LDS float a lane reads for a tap is the one the staging
// filled from that tap's pixel (or a zero, where the pixel lies outside the image), that a window's address has the alignment
// class the kernel's reads assume, and the reciprocal-multiply divisions against real ones.
//   c++ -O2 -std=c++17 -fsanitize=address,undefined -o dwconv_dil_f32_geom_check scripts/dwconv_dil_f32_geom_check.cpp
//   ./dwconv_dil_f32_geom_check                              the lists below
//   ./dwconv_dil_f32_geom_check N,C,H,W,R,d,pad ...          these shapes instead
// (tests/test_atrous_f32_cpu.py runs it.)  The walk below is the kernel's own: same plan, same grid, same workgroup -> tiles,
// same lane -> strips, the same predicates in front of every access.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_dwconv_dil_f32_geom.h"

using namespace fq;

struct Shape { int N, C, H, W, R, d, pad; };

static void fail(const char* what, const Shape& s) {
    printf("%s: N %d, C %d, H %d, W %d, %dx%d dilation %d, pad %d\n", what, s.N, s.C, s.H, s.W, s.R, s.R, s.d, s.pad);
    exit(1);
}

static long run(const Shape& s, bool hist) {
    DdfGeom g;
    if (!ddf_plan(g, s.N, s.C, s.H, s.W, s.R, s.d, s.pad)) fail("the plan declines a shape of the list", s);
    const int R = s.R;
    const size_t in_elems = (size_t)s.N * s.C * s.H * s.W, out_elems = (size_t)s.N * s.C * g.Ho * g.Wo;
    const size_t lds = (size_t)kDdfZero + g.fill;
    if (lds > (size_t)kDdfLdsFloats || g.PP > kDdfMaxPP || g.PP < 1 || g.TH < 1 || g.TQ < 1 || g.TQ > kDdfMaxTQ || (g.pitch & 3) ||
        g.strips != (unsigned)(g.PP * g.TH * g.TQ) || g.RB * g.TH < g.Ho || g.CB * g.TQ * kDdfStrip < g.Wo)
        fail("tile larger than its LDS, or tiles that do not cover the plane", s);
    if (in_elems >= (1ul << 30) || out_elems >= (1ul << 30)) fail("32-bit offset arithmetic wraps", s);
    std::vector<unsigned char> written(out_elems, 0);
    std::vector<long> src(lds, -1);                       // what each LDS float holds: element offset of x, or -1 for zero
    const unsigned G = ddf_grid(g, hist);
    long loads = 0;
    for (unsigned b = 0; b < G; ++b) {
        for (unsigned tile = geom_first_tile(b, G); tile < g.tiles; tile += G) {
            const DdfTilePos tp = ddf_tile_pos(g, tile);
            if (tp.plane0 >= g.planes || tp.oh0 >= g.Ho || tp.ow0 >= g.Wo || (tp.cb0 & 3) || tp.base[kDdfMaxR] > g.NR)
                fail("tile outside the tensor, or more staged rows than a slot has", s);
            for (unsigned e = 0; e < g.fill; ++e) {       // (lane e % 256 in step e / 256: every e < fill exactly once)
                unsigned off = 0;
                const bool ld = ddf_fill_src(g, tp, e, &off);
                const unsigned pi = e / g.slot, rem = e % g.slot, sr = rem / g.pitch;
                if (geom_mulhi(e, g.m_slot) != pi || geom_mulhi(rem, g.m_pitch) != sr) fail("reciprocal division is off", s);
                if (ld) {
                    if ((size_t)off >= in_elems) fail("staged element outside the input", s);
                    if (tp.plane0 + pi >= g.planes || off / ((unsigned)s.H * s.W) != tp.plane0 + pi) fail("staged element of another plane", s);
                    ++loads;
                }
                src[kDdfZero + e] = ld ? (long)off : -1;
            }
            for (unsigned u = 0; u < g.strips; ++u) {     // (lane u % 256 in step u / 256)
                const DdfStripPos lp = ddf_strip_pos(g, u);
                const unsigned per = (unsigned)(g.TH * g.TQ);
                if (lp.pi != (int)(u / per) || lp.t != (int)(u % per / g.TQ) || lp.q != (int)(u % per % g.TQ))
                    fail("reciprocal division of the strip index is off", s);
                const int cnt = ddf_out_count(g, tp, lp);
                if (cnt == 0) continue;
                const long plane = (long)tp.plane0 + lp.pi, oh = tp.oh0 + lp.t, ow = tp.ow0 + lp.q * kDdfStrip;
                for (int r = 0; r < R; ++r) {
                    const int row = ddf_row_off(g, tp, lp.t, r);
                    for (int t = 0; t < R; ++t) {
                        const unsigned rd = ddf_read_index(g, lp.pi, row, ddf_win_col(g, tp, lp.q, t), t);
                        if ((size_t)rd + kDdfStrip > lds) fail("LDS read outside the staged rows and the zero row", s);
                        if (rd < (unsigned)kDdfZero && rd + kDdfStrip > (unsigned)kDdfZero) fail("zero-row read runs into the staged rows", s);
                        if ((int)(rd & 3u) != g.cls[t]) fail("LDS read not of its alignment class", s);
                        for (int j = 0; j < cnt; ++j) {
                            const long ih = oh - s.pad + (long)r * s.d, iw = ow + j - s.pad + (long)t * s.d;
                            const bool in = ih >= 0 && ih < s.H && iw >= 0 && iw < s.W;
                            const long want = in ? (plane * s.H + ih) * s.W + iw : -1;
                            if (src[rd + j] != want) fail("a tap reads another pixel's LDS float", s);
                        }
                    }
                }
                const unsigned o = ddf_out_off(g, tp, lp);
                for (int j = 0; j < cnt; ++j) {
                    if ((size_t)o + j >= out_elems) fail("store outside the output", s);
                    if ((long)o + j != (plane * g.Ho + oh) * g.Wo + ow + j) fail("store to the wrong element", s);
                    if (written[(size_t)o + j]++) fail("output element written twice", s);
                }
            }
        }
    }
    for (unsigned char v : written)
        if (v != 1) fail("output element not written", s);
    return loads;
}

int main(int argc, char** argv) {
    long total = 0;
    if (argc > 1) {
        for (int a = 1; a < argc; ++a) {
            Shape s;
            if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d", &s.N, &s.C, &s.H, &s.W, &s.R, &s.d, &s.pad) != 7) {
                printf("cannot read case %s\n", argv[a]);
                return 2;
            }
            for (bool hist : {false, true}) total += run(s, hist);
        }
        printf("ok, %ld loads\n", total);
        return 0;
    }
    // tests/atrous_f32_cases.py: SHAPES
    const Shape tests[] = {{2, 3, 5, 7, 3, 2, 2},     {1, 5, 14, 14, 3, 6, 6},  {2, 4, 14, 14, 3, 12, 12}, {2, 4, 14, 14, 3, 18, 18},
                           {1, 2, 9, 11, 5, 2, 4},    {1, 2, 20, 9, 3, 3, 0},   {1, 3, 12, 10, 3, 4, 1},   {1, 2, 6, 6, 3, 2, 4},
                           {1, 2, 70, 33, 3, 2, 2},   {3, 130, 7, 7, 3, 2, 2},  {1, 1, 3, 5, 3, 64, 64},   {1, 1, 200, 33, 3, 2, 2},
                           {1, 1, 40, 300, 3, 20, 20}};
    // the atrous depthwise layers of DeepLabV3Plus_fabu at 224 x 224: output stride 16 (d = 2 on 14 x 14, ASPP at 6 / 12 / 18) and
    // output stride 8 (d = 2 and 4 on 28 x 28, ASPP at 12 / 24 / 36); then planes that need row bands of both kinds (TH >= d and
    // TH < d), column blocks, 5x5 at the largest dilation, and more tiles than either grid has workgroups
    const Shape net[] = {{1, 96, 14, 14, 3, 2, 2},    {1, 320, 14, 14, 3, 6, 6}, {1, 320, 14, 14, 3, 12, 12}, {1, 320, 14, 14, 3, 18, 18},
                         {1, 64, 28, 28, 3, 2, 2},    {1, 160, 28, 28, 3, 4, 4}, {1, 320, 28, 28, 3, 12, 12}, {1, 320, 28, 28, 3, 24, 24},
                         {1, 320, 28, 28, 3, 36, 36}, {1, 2, 200, 120, 3, 2, 2}, {1, 1, 300, 400, 5, 64, 128}, {1, 1, 40, 700, 3, 5, 3},
                         {1, 1, 90, 1100, 5, 64, 256}, {1, 1, 600, 9, 3, 7, 7},  {300, 131, 7, 7, 3, 2, 2},   {2, 3, 129, 130, 5, 3, 6}};
    for (const Shape& s : tests)
        for (bool hist : {false, true}) total += run(s, hist);
    for (const Shape& s : net)
        for (bool hist : {false, true}) total += run(s, hist);
    // every padding and alignment class of both kernels at an odd size
    for (int R : {3, 5})
        for (int d : {2, 3, 5})
            for (int pad = 0; pad <= d * (R - 1); ++pad)
                if (21 + 2 * pad >= d * (R - 1) + 1) total += run({2, 5, 21, 23, R, d, pad}, false);
    printf("ok, %ld loads\n", total);
    return 0;
}
