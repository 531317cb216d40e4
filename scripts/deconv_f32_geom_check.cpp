// Host check of the transposed fp32 kernel's address arithmetic (csrc/fq_deconv_f32_geom.h): over the GPU tests' shapes and the
// up-convolutions of model/unet/UNet_fabu.py (base width 32, depth 4, up_kernel 2 and 4, 224 x 224) at N = 1, every lane of every
// launch (the plain grid and the histogram form's smaller one) loads inside x and wt, stores inside y, and every output element is
// written exactly once.  It also checks, against the layer's definition in plain 64-bit arithmetic, that the taps a lane walks for
// an output are exactly the taps (r, s) with (oh + pad - r) % stride == 0 and (ow + pad - s) % stride == 0, in ascending order,
// that each reads the pixel ((oh + pad - r) / stride, (ow + pad - s) / stride) of its image or is "outside: zero", and that the
// weight offset is that of (r, s, c, k) in wt [(r*S + s)*Cin + c][Cout].
//   c++ -O2 -std=c++17 -o deconv_f32_geom_check scripts/deconv_f32_geom_check.cpp && ./deconv_f32_geom_check
// (tests/test_deconv_f32_cpu.py runs it, built with -fsanitize=address,undefined.)  The walk below is the kernel's own: same
// plan, same grid, same workgroup -> work items, same wave and lane -> channels and column, the same predicates in front of
// every access.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_deconv_f32_geom.h"

using namespace fq;

struct Shape { int N, Cin, Cout, H, W, R, S, stride, pad, outpad; };

static void fail(const char* what, const Shape& s) {
    printf("%s: N %d, %d -> %d channels, H %d, W %d, %dx%d stride %d, pad %d, output padding %d\n", what, s.N, s.Cin, s.Cout, s.H,
           s.W, s.R, s.S, s.stride, s.pad, s.outpad);
    exit(1);
}

static long run(const Shape& s, bool hist) {
    DcGeom g;
    if (!dc_supported(s.Cin, s.Cout, 1, s.R, s.S, s.stride, s.stride, s.pad, s.pad, s.outpad, s.outpad, 1, 1, s.H, s.W) ||
        !dc_plan(g, s.N, s.Cin, s.H, s.W, s.Cout, s.R, s.S, s.stride, s.pad, s.outpad))
        fail("the plan declines a shape of the list", s);
    const long Ho = (long)(s.H - 1) * s.stride - 2L * s.pad + s.R + s.outpad, Wo = (long)(s.W - 1) * s.stride - 2L * s.pad + s.S + s.outpad;
    if (g.Ho != Ho || g.Wo != Wo || g.MW * g.NW * 64 != kDcBlock) fail("the plan's output plane or wave grid is off", s);
    const size_t in_elems = (size_t)s.N * s.Cin * s.H * s.W, out_elems = (size_t)s.N * s.Cout * Ho * Wo;
    const size_t w_elems = (size_t)s.R * s.S * s.Cin * s.Cout;
    if (in_elems >= (1UL << 30) || out_elems >= (1UL << 30) || w_elems >= (1UL << 30) ||
        (unsigned long)g.items + kDcMaxBlocks > 0xffffffffUL)
        fail("32-bit item or offset arithmetic wraps", s);
    std::vector<unsigned char> written(out_elems, 0);
    const unsigned G = dc_grid(g, hist);
    if (G < 1 || G > (unsigned)(hist ? kDcMaxBlocksHist : kDcMaxBlocks)) fail("grid outside its cap", s);
    long loads = 0;
    for (unsigned b = 0; b < G; ++b) {
        for (unsigned item = geom_first_tile(b, G); item < g.items; item += G) {
            const DcItemPos ip = dc_item_pos(g, item);
            if (ip.rp < 0 || ip.rp >= s.stride || g.Hq[ip.rp] < 1 || item < g.item0[ip.rp] || item >= g.item0[ip.rp + 1] ||
                ip.m0 >= (unsigned)s.Cout || ip.j0 >= g.cols[ip.rp])
                fail("work item outside the layer", s);
            for (unsigned tid = 0; tid < (unsigned)kDcBlock; ++tid) {
                const unsigned lane = tid & 63u, wave = tid / 64u, l32 = lane & 31u, h = lane >> 5;
                const unsigned mbase = ip.m0 + dc_wave_m(g, wave);
                if (mbase >= (unsigned)s.Cout) continue;
                const unsigned j = ip.j0 + dc_wave_j(g, wave) + l32;
                const DcColPos col = dc_col_pos(g, ip.rp, j);
                if (col.valid != (j < g.cols[ip.rp])) fail("column predicate is off", s);
                if (col.valid && ((long)((col.n * (unsigned long)g.Hq[ip.rp] + col.ohq) * g.Qmax + col.q) != (long)j || col.n >= (unsigned)s.N ||
                                  col.ohq >= g.Hq[ip.rp] || col.q >= g.Qmax))
                    fail("column -> (image, row, column) is off", s);
                const long oh = ip.rp + (long)col.ohq * s.stride;
                const unsigned ka = mbase + l32;
                // the K loop: the taps of this lane's column for every column phase, and the weights of this lane's channel
                for (int cp = 0; cp < s.stride; ++cp) {
                    const long ow = cp + (long)col.q * s.stride;
                    int want_r = 0;                                       // the next r the definition expects, ascending
                    for (int r = dc_first_tap(g, ip.rp); r < s.R; r += s.stride) {
                        while (want_r < s.R && (oh + s.pad - want_r) % s.stride != 0) ++want_r;
                        if (col.valid && want_r != r) fail("a kernel row of the phase is skipped or out of order", s);
                        ++want_r;
                        int want_s = 0;
                        for (int t = dc_first_tap(g, cp); t < s.S; t += s.stride) {
                            while (want_s < s.S && (ow + s.pad - want_s) % s.stride != 0) ++want_s;
                            if (col.valid && want_s != t) fail("a kernel column of the phase is skipped or out of order", s);
                            ++want_s;
                            unsigned off = 0;
                            const bool ld = dc_tap_src(g, col, ip.rp, cp, r, t, &off);
                            const long ihn = oh + s.pad - r, iwn = ow + s.pad - t;
                            const bool in = col.valid && ihn >= 0 && iwn >= 0 && ihn % s.stride == 0 && iwn % s.stride == 0 &&
                                            ihn / s.stride < s.H && iwn / s.stride < s.W;
                            if (ld != in) fail("tap predicate is off", s);
                            if (ld) {
                                const size_t last = (size_t)off + (size_t)(s.Cin - 2 + h) * g.plane_in;      // the lane's last channel
                                if (last >= in_elems) fail("load outside the input", s);
                                if ((long)off != (((long)col.n * s.Cin) * s.H + ihn / s.stride) * s.W + iwn / s.stride)
                                    fail("load of the wrong pixel", s);
                                loads += s.Cin / 2;
                            }
                            if (ka < (unsigned)s.Cout) {
                                const unsigned w0 = dc_w_off(g, r, t, h, ka);
                                const size_t wl = (size_t)w0 + (size_t)(s.Cin - 2) * s.Cout;
                                if (wl >= w_elems) fail("load outside the weights", s);
                                if ((long)w0 != ((long)(r * s.S + t) * s.Cin + h) * s.Cout + ka) fail("load of the wrong weight", s);
                                loads += s.Cin / 2;
                            }
                        }
                        while (want_s < s.S && (ow + s.pad - want_s) % s.stride != 0) ++want_s;
                        if (col.valid && want_s < s.S) fail("a kernel column of the phase is missing", s);
                    }
                    while (want_r < s.R && (oh + s.pad - want_r) % s.stride != 0) ++want_r;
                    if (col.valid && want_r < s.R) fail("a kernel row of the phase is missing", s);
                }
                // the epilogue
                const int cnt = dc_out_count(g, col);
                if (cnt < 0 || cnt > s.stride || (col.valid && cnt < 1)) fail("count of existing column phases is off", s);
                for (int e = 0; e < 16; ++e) {
                    const unsigned k = mbase + dc_acc_row(e, h);
                    if (dc_acc_row(e, h) >= 32u) fail("accumulator row outside the MFMA tile", s);
                    if (k >= (unsigned)s.Cout || cnt == 0) continue;
                    const unsigned o = dc_out_off(g, col, ip.rp, k);
                    for (int cp = 0; cp < cnt; ++cp) {
                        const long ow = cp + (long)col.q * s.stride;
                        if (ow >= Wo || oh >= Ho) fail("store outside the output plane", s);
                        if ((size_t)o + cp >= out_elems) fail("store outside the output", s);
                        if ((long)o + cp != (((long)col.n * s.Cout + k) * Ho + oh) * Wo + ow) fail("store to the wrong element", s);
                        if (written[(size_t)o + cp]++) fail("output element written twice", s);
                    }
                }
            }
        }
    }
    for (unsigned char v : written)
        if (v != 1) fail("output element not written", s);
    return loads;
}

int main() {
    // tests/deconv_f32_util.py: SHAPES
    const Shape tests[] = {{1, 16, 4, 1, 1, 2, 2, 2, 0, 0},  {1, 16, 4, 1, 1, 1, 1, 2, 0, 1},  {2, 16, 8, 3, 5, 2, 2, 2, 0, 0},
                           {1, 16, 4, 5, 7, 4, 4, 2, 1, 0},  {1, 16, 4, 5, 7, 3, 3, 2, 1, 1},  {1, 16, 4, 4, 4, 3, 3, 1, 1, 0},
                           {1, 32, 4, 3, 3, 2, 3, 3, 1, 2},  {1, 16, 4, 2, 2, 8, 8, 4, 7, 3},  {1, 48, 40, 4, 4, 2, 2, 2, 0, 0},
                           {1, 16, 132, 3, 3, 2, 2, 2, 0, 0}, {3, 16, 4, 2, 70, 2, 2, 2, 0, 0}, {4, 16, 4, 130, 130, 1, 1, 4, 0, 0}};
    // the four up-convolutions of UNet(base_width 32, depth 4, up="deconv") at 224 x 224, up_kernel 2 and 4
    const Shape net[] = {{1, 512, 256, 14, 14, 2, 2, 2, 0, 0}, {1, 256, 128, 28, 28, 2, 2, 2, 0, 0}, {1, 128, 64, 56, 56, 2, 2, 2, 0, 0},
                         {1, 64, 32, 112, 112, 2, 2, 2, 0, 0}, {1, 512, 256, 14, 14, 4, 4, 2, 1, 0}, {1, 256, 128, 28, 28, 4, 4, 2, 1, 0},
                         {1, 128, 64, 56, 56, 4, 4, 2, 1, 0},  {1, 64, 32, 112, 112, 4, 4, 2, 1, 0}};
    long total = 0;
    for (const Shape& s : tests)
        for (bool hist : {false, true}) total += run(s, hist);
    for (const Shape& s : net)
        for (bool hist : {false, true}) total += run(s, hist);
    // every stride with every padding and output padding of a 3 x 4 and a 5 x 2 kernel on an odd plane, three images, a partly
    // filled channel tile
    for (int stride = 1; stride <= kDcMaxStride; ++stride)
        for (int pad = 0; pad < 2; ++pad)
            for (int outpad = 0; outpad < stride; ++outpad) {
                total += run({3, 16, 36, 5, 9, 3, 4, stride, pad, outpad}, false);
                total += run({2, 32, 68, 7, 3, 5, 2, stride, pad, outpad}, true);
            }
    printf("ok, %ld loads\n", total);
    return 0;
}
