// Host check of the grouped kernel's index arithmetic (csrc/fq_gconv_i8_geom.h): every lane of every launch over the GPU tests'
// shapes and the ResNeXt model's grouped layers at N = 1, on a model of memory in which each byte is its own address.
//   c++ -O2 -std=c++17 -o gconv_geom_check scripts/gconv_geom_check.cpp && ./gconv_geom_check
//   ./gconv_geom_check --list      prints the shape list, one "G Cgi Cgo R stride pad N H W" per line, and walks nothing
//   ./gconv_geom_check window=T G,Cgi,Cgo,R,stride,pad,N,H,W    a size-limit row instead of the list: every workgroup and lane, but
//                                  only the first and the last T strip blocks of the launch (neither activation reaches 2^31 bytes:
//                                  there is no boundary between); the 32-bit strip and offset arithmetic must not wrap
// (tests/test_grouped_plan_cpu.py runs both and compares the list with the GPU tests' own.)  The walk below is the kernel's own:
// same launch size, same workgroup -> (channel block, strip blocks), same lane -> (quad, strip), the same predicates in front
// of every access.  It exits non-zero on a load outside the input or the packed weights, an LDS index outside the staged block
// (or an LDS slot staged twice or not at all), a tap that reads another pixel, channel or weight than the rule's, a tap inside
// the image that is skipped, a store outside the output, an output dword written twice or not at all, and a wrong
// padding-channel mask.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_gconv_i8_geom.h"

using namespace fq;

struct Shape { int G, Cgi, Cgo, R, stride, pad, N, H, W; };

static void fail(const char* what, const Shape& s) {
    printf("%s: G %d, Cgi %d, Cgo %d, %dx%d stride %d pad %d, N %d, H %d, W %d\n", what, s.G, s.Cgi, s.Cgo, s.R, s.R, s.stride,
           s.pad, s.N, s.H, s.W);
    exit(1);
}

// The packed weights as include/fq.h describes them, built without the header's functions: entry b of the buffer names the
// weight (k, j, t) it holds as (k * Cgi + j) * RS + t, or -1 in a padding quad.
static std::vector<long> pack_ids(int K, int Kpad, int Cgi, int RS) {
    std::vector<long> ids((size_t)Kpad * RS * Cgi, -2);
    size_t b = 0;
    for (int kq = 0; kq < Kpad / 4; ++kq)
        for (int t = 0; t < RS; ++t)
            for (int j4 = 0; j4 < Cgi / 4; ++j4)
                for (int i = 0; i < 4; ++i)
                    for (int c = 0; c < 4; ++c, ++b) {
                        const int k = 4 * kq + i, j = 4 * j4 + c;
                        ids[b] = k < K ? ((long)k * Cgi + j) * RS + t : -1;
                    }
    return ids;
}

static unsigned long g_window = 0;          // window=T: strip blocks [T, sblocks - T) are skipped

static long run(const Shape& s) {
    const int R = s.R, STRIDE = s.stride, C = s.G * s.Cgi, K = s.G * s.Cgo;
    if (s.H + 2 * s.pad < R || s.W + 2 * s.pad < R) return 0;
    GcGeom g;
    if (!gc_setup(g, s.N, s.H, s.W, C, K, s.G, R, STRIDE, s.pad, s.pad)) fail("launch does not fit", s);
    if (g.Cpad % 16 || g.Kpad % 16 || g.Cpad < C || g.Kpad < K || g.Kpad != g.KBn * g.KB4 * 4 || kGcBlock % g.KB4)
        fail("bad derived geometry", s);
    const int NPIX = (kGcTQ - 1) * STRIDE + R;
    const size_t in_bytes = (size_t)s.N * s.H * s.W * g.Cpad, out_bytes = (size_t)s.N * g.P * g.Q * g.Kpad;
    const size_t w_bytes = (size_t)g.Kpad * g.RS * g.Cgi;
    const std::vector<long> wid = pack_ids(K, g.Kpad, g.Cgi, g.RS);
    if (g.units * (size_t)kGcUnit * g.KBn != w_bytes || g.units * (size_t)kGcUnit > 36864) fail("staged block size", s);
    const unsigned blocks = gc_blocks(g);
    if (blocks == 0 || blocks > (unsigned)kGcMaxBlocks || blocks % g.KBn) fail("launch size", s);
    const unsigned step = gc_sb_step(g, blocks);
    if (in_bytes > 0xffffffffUL || out_bytes > 0xffffffffUL || (unsigned long)g.sblocks * g.SPW + kGcBlock > 0xffffffffUL ||
        (unsigned long)g.sblocks + step > 0xffffffffUL || (unsigned long)s.N * g.P * g.QS != g.strips)
        fail("32-bit strip or offset arithmetic wraps", s);
    const bool windowed = g_window && (unsigned long)g.sblocks > 2 * g_window;
    std::vector<bool> written(out_bytes / 4, false);
    std::vector<long> lds(g.units);
    long checked = 0;
    for (unsigned b = 0; b < blocks; ++b) {
        const int kb = gc_block_kb(g, b);
        if (kb < 0 || kb >= g.KBn) fail("channel block out of range", s);
        // staging: every thread copies units tid, tid + 256, ...
        std::fill(lds.begin(), lds.end(), -1L);
        for (unsigned i = 0; i < g.units; ++i) {
            const unsigned src = gc_stage_src(g, kb, i), dst = gc_stage_dst(g, i);
            if (((size_t)src + 1) * kGcUnit > w_bytes) fail("weight load outside the packed weights", s);
            if (dst >= g.units) fail("LDS store outside the staged block", s);
            if (lds[dst] != -1) fail("LDS slot staged twice", s);
            lds[dst] = src;
        }
        for (long v : lds)
            if (v < 0) fail("LDS slot not staged", s);
        for (int lane = 0; lane < kGcBlock; ++lane) {
            const int kql = gc_lane_quad(g, lane), ls = gc_lane_strip(g, lane);
            if (kql < 0 || kql >= g.KB4 || ls < 0 || ls >= g.SPW) fail("lane split out of range", s);
            const int kq = gc_quad(g, kb, kql);
            if (kq < 0 || 4 * kq + 3 >= g.Kpad) fail("output quad out of range", s);
            const bool valid = gc_quad_valid(g, kq);
            if (valid != (4 * kq + 3 < K)) fail("wrong padding-channel mask", s);
            for (unsigned sb = gc_block_sb0(g, b); sb < g.sblocks; sb += step) {
                if (windowed && sb >= g_window && sb < g.sblocks - g_window) {   // jump to this workgroup's first block of the last window
                    const unsigned long steps = ((unsigned long)(g.sblocks - g_window) - sb + step - 1) / step;
                    const unsigned long next = sb + steps * step;
                    if (next >= g.sblocks) break;
                    sb = (unsigned)(next - step);
                    continue;
                }
                const unsigned strip = sb * (unsigned)g.SPW + (unsigned)ls;
                if (strip >= g.strips) continue;
                const GcStripPos sp = gc_strip_pos(g, strip);
                if (sp.n < 0 || sp.n >= s.N || sp.p < 0 || sp.p >= g.P || sp.q0 < 0 || sp.q0 >= g.Q) fail("strip out of range", s);
                const int ih0 = sp.p * STRIDE - s.pad, iw0 = sp.q0 * STRIDE - s.pad;
                if (valid) {
                    for (int j4 = 0; j4 < g.CH; ++j4) {
                        const int chan = gc_in_chan(g, kq, j4);
                        const int want_chan = (4 * kq / s.Cgo) * s.Cgi + 4 * j4;     // group of the quad's channels, chunk j4
                        if ((4 * kq + 3) / s.Cgo != 4 * kq / s.Cgo) fail("a quad spans two groups", s);
                        if (chan != want_chan || chan + 3 >= C) fail("tap reads another channel", s);
                        for (int r = 0; r < R; ++r) {
                            const int ih = ih0 + r;
                            // the loads: one dword per input column of the strip, predicated on the image bounds only
                            std::vector<long> xv(NPIX, -1);
                            for (int k = 0; k < NPIX; ++k) {
                                const int iw = iw0 + k;
                                const bool inside = ih >= 0 && ih < s.H && iw >= 0 && iw < s.W;
                                if (gc_in_ok(g, ih, iw) != inside) fail(inside ? "tap inside the image is skipped" : "tap outside the image is loaded", s);
                                if (!inside) continue;
                                const unsigned o = gc_in_off(g, sp.n, ih, iw, chan);
                                if ((size_t)o + 4 > in_bytes || o % 4) fail("load outside the input", s);
                                xv[k] = o;                                           // each byte is its own address
                                ++checked;
                            }
                            for (int ss = 0; ss < R; ++ss) {
                                const int t = r * R + ss;
                                const unsigned lu = gc_lds_unit(g, kql, t, j4);
                                if (lu >= g.units) fail("LDS read outside the staged block", s);
                                const size_t wb = (size_t)lds[lu] * kGcUnit;
                                if (gc_w_unit(g, kq, t, j4) != (unsigned)lds[lu]) fail("LDS slot holds another unit", s);
                                for (int i = 0; i < 4; ++i)
                                    for (int c = 0; c < 4; ++c)
                                        if (wid[wb + 4 * i + c] != ((long)(4 * kq + i) * s.Cgi + 4 * j4 + c) * g.RS + t)
                                            fail("tap reads another weight", s);
                                for (int j = 0; j < kGcTQ; ++j) {
                                    const int qq = sp.q0 + j, iw = qq * STRIDE - s.pad + ss;
                                    const bool inside = ih >= 0 && ih < s.H && iw >= 0 && iw < s.W;
                                    const long got = xv[j * STRIDE + ss];
                                    const long want = inside ? (((long)sp.n * s.H + ih) * s.W + iw) * g.Cpad + want_chan : -1;
                                    if (got != want) fail("tap reads another pixel", s);
                                }
                            }
                        }
                    }
                }
                for (int j = 0; j < kGcTQ; ++j) {
                    if (gc_out_ok(g, sp.q0 + j) != (sp.q0 + j < g.Q)) fail("store predicate", s);
                    if (!gc_out_ok(g, sp.q0 + j)) continue;
                    const unsigned o = gc_out_off(g, sp.n, sp.p, sp.q0 + j, kq);
                    if ((size_t)o + 4 > out_bytes || o % 4) fail("store outside the output", s);
                    if ((long)o != (((long)sp.n * g.P + sp.p) * g.Q + sp.q0 + j) * g.Kpad + 4 * kq) fail("store to another pixel", s);
                    if (written[o / 4]) fail("output dword written twice", s);
                    written[o / 4] = true;
                }
            }
        }
    }
    if (!windowed) {
        for (bool v : written)
            if (!v) fail("output dword not written", s);
    } else {                                              // every output of the whole images that the two windows cover
        const size_t img = (size_t)g.P * g.Q * g.Kpad / 4, imgs = g_window * g.SPW / ((size_t)g.P * g.QS);
        if (imgs < 1) fail("window smaller than one image", s);
        for (size_t i = 0; i < imgs * img; ++i)
            if (!written[i] || !written[written.size() - 1 - i]) fail("output dword of the first or last images not written", s);
    }
    return checked;
}

int main(int argc, char** argv) {
    const bool list = argc > 1 && !strcmp(argv[1], "--list");
    if (argc > 1 && !list) {
        long total = 0;
        for (int a = 1; a < argc; ++a) {
            Shape s;
            if (strncmp(argv[a], "window=", 7) == 0) { g_window = strtoul(argv[a] + 7, nullptr, 10); continue; }
            if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d,%d,%d", &s.G, &s.Cgi, &s.Cgo, &s.R, &s.stride, &s.pad, &s.N, &s.H, &s.W) != 9) {
                printf("cannot read case %s\n", argv[a]);
                return 2;
            }
            total += run(s);
        }
        printf("ok, %ld loads checked\n", total);
        return 0;
    }
    std::vector<Shape> shapes;
    // the GPU tests' list (tests/grouped_doubles.py: kernel_shapes())
    const int groups[][3] = {{2, 4, 4}, {8, 4, 4}, {3, 8, 4}, {2, 16, 8}, {2, 32, 32}, {2, 64, 64}, {5, 4, 12}, {32, 4, 4}};
    const int planes[][2] = {{1, 1}, {2, 2}, {5, 7}, {9, 11}, {33, 17}};
    for (const auto& gr : groups)
        for (int R : {1, 3})
            for (int stride : {1, 2})
                for (int pad = 0; pad < R; ++pad)
                    for (const auto& hw : planes)
                        for (int N : {1, 3}) shapes.push_back({gr[0], gr[1], gr[2], R, stride, pad, N, hw[0], hw[1]});
    shapes.push_back({32, 4, 4, 3, 1, 1, 8, 112, 112});       // more tiles than workgroups: the step over strip blocks
    const size_t listed = shapes.size();
    // the grouped layers of model/resnext/ResNeXt_fabu.py (32x4d, 224 x 224) at N = 1
    const int model[][5] = {{4, 4, 1, 56, 56}, {8, 8, 2, 56, 56}, {8, 8, 1, 28, 28}, {16, 16, 2, 28, 28}, {16, 16, 1, 14, 14},
                            {32, 32, 2, 14, 14}, {32, 32, 1, 7, 7}};
    for (const auto& m : model) shapes.push_back({32, m[0], m[1], 3, m[2], 1, 1, m[3], m[4]});
    if (list) {
        for (size_t i = 0; i < listed; ++i) {
            const Shape& s = shapes[i];
            printf("%d %d %d %d %d %d %d %d %d\n", s.G, s.Cgi, s.Cgo, s.R, s.stride, s.pad, s.N, s.H, s.W);
        }
        return 0;
    }
    long total = 0;
    for (const Shape& s : shapes) total += run(s);
    printf("ok, %zu shapes, %ld loads checked\n", shapes.size(), total);
    return 0;
}
