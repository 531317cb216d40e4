// Host check of the atrous depthwise kernel's address arithmetic (csrc/fq_dwconv_dil_i8_geom.h): every lane of every launch
// loads inside the input, stores inside the output, and every output dword is written exactly once.
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -o dwconv_dil_geom_check scripts/dwconv_dil_geom_check.cpp
//   ./dwconv_dil_geom_check                                  a built-in sweep
//   ./dwconv_dil_geom_check R,d,N,H,W,C,pad_h,pad_w ...      these launches instead (tests/test_atrous_plan_cpu.py passes the
//                                                            shapes of tests/test_gpu_atrous_depthwise_i8.py)
// The walk below is the kernel's own: same launch size, same lane -> (channel group, first tile, tile stride), the digits
// advanced with dwd_advance and held against dwd_decode of the tile number, the same lattice rows and columns per tile, the
// same predicates in front of every access.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_dwconv_dil_i8_geom.h"

using namespace fq;

struct Case { int R, d, N, H, W, C, pad_h, pad_w; };

static void fail(const char* what, const Case& c) {
    printf("%s: %dx%d dilation %d, N %d, H %d, W %d, C %d, pad %d,%d\n", what, c.R, c.R, c.d, c.N, c.H, c.W, c.C, c.pad_h, c.pad_w);
    exit(1);
}

template <int R>
long run(const Case& c) {
    constexpr int TP = DwTile<R>::TP, NROWS = TP - 1 + R, NPIX = kDwTQ - 1 + R;
    const int span = c.d * (R - 1);
    if (c.d < kDwDilMin || c.d > kDwDilMax || c.pad_h > span || c.pad_w > span || c.H + 2 * c.pad_h <= span || c.W + 2 * c.pad_w <= span)
        return 0;                                                     // (what the entry point declines)
    const int Cpad = (c.C + 15) / 16 * 16;
    DwDilGeom a;
    if (!dwd_make(a, TP, c.N, c.H, c.W, Cpad, R, c.d, c.pad_h, c.pad_w)) fail("the launch does not fit 32-bit tile arithmetic", c);
    const DwGeom& g = a.g;
    if (g.P != c.H + 2 * c.pad_h - span || g.Q != c.W + 2 * c.pad_w - span) fail("output plane", c);
    const unsigned threads = dwd_blocks(a) * kDwBlock, sp_stride = threads / g.C4;
    const size_t in_bytes = (size_t)c.N * c.H * c.W * Cpad, out_bytes = (size_t)c.N * g.P * g.Q * Cpad;
    if ((unsigned long)g.tiles + sp_stride > 0xffffffffUL || in_bytes > 0xffffffffUL || out_bytes > 0xffffffffUL)
        fail("32-bit tile or offset arithmetic wraps", c);
    std::vector<unsigned char> written(out_bytes / 4, 0);
    long checked = 0;
    for (unsigned gid = 0; gid < threads; ++gid) {
        const int c4 = gid % g.C4;
        unsigned tile = gid / g.C4;
        if (tile >= sp_stride) continue;
        DwDilPos pos = dwd_decode(a, tile);
        const DwDilPos step = dwd_decode(a, sp_stride);
        for (; tile < g.tiles; tile += sp_stride, dwd_advance(a, pos, step)) {
            const DwDilPos want = dwd_decode(a, tile);
            if (pos.n != want.n || pos.pb != want.pb || pos.fh != want.fh || pos.qb != want.qb || pos.fw != want.fw)
                fail("advanced digits are not the tile's", c);
            if (pos.n < 0 || pos.n >= c.N || pos.fh >= a.d || pos.fw >= a.d) fail("tile digits out of range", c);
            const DwDilTile tl = dwd_tile<TP>(a, pos);
            if (!dw_out_ok(g, tl.p0, tl.q0)) continue;
            for (int i = 0; i < NROWS; ++i) {
                for (int k = 0; k < NPIX; ++k) {
                    const int ih = tl.ih0 + i * a.d, iw = tl.iw0 + k * a.d;
                    if (!dw_in_ok(g, ih, iw)) continue;
                    const size_t o = dw_in_off(g, pos.n, ih, iw, c4);
                    if (o + 4 > in_bytes) fail("load outside the input", c);
                    if (o != (((size_t)pos.n * c.H + ih) * c.W + iw) * Cpad + 4u * c4) fail("input offset is not the pixel's", c);
                    ++checked;
                }
            }
            for (int t = 0; t < TP; ++t) {
                for (int j = 0; j < kDwTQ; ++j) {
                    const int p = tl.p0 + t * a.d, q = tl.q0 + j * a.d;
                    if (!dw_out_ok(g, p, q)) continue;
                    if (p % a.d != pos.fh || q % a.d != pos.fw) fail("output pixel of another phase", c);
                    const size_t o = dw_out_off(g, pos.n, p, q, c4);
                    if (o + 4 > out_bytes || o % 4) fail("store outside the output", c);
                    if (o != (((size_t)pos.n * g.P + p) * g.Q + q) * Cpad + 4u * c4) fail("output offset is not the pixel's", c);
                    if (written[o / 4]) fail("output dword written twice", c);
                    written[o / 4] = 1;
                }
            }
        }
    }
    for (unsigned char v : written)
        if (!v) fail("output dword not written", c);
    return checked;
}

static long run_case(const Case& c) { return c.R == 3 ? run<3>(c) : run<5>(c); }

int main(int argc, char** argv) {
    long total = 0;
    if (argc > 1) {
        for (int i = 1; i < argc; ++i) {
            Case c;
            if (sscanf(argv[i], "%d,%d,%d,%d,%d,%d,%d,%d", &c.R, &c.d, &c.N, &c.H, &c.W, &c.C, &c.pad_h, &c.pad_w) != 8 || (c.R != 3 && c.R != 5)) {
                printf("cannot read case %s\n", argv[i]);
                return 2;
            }
            const long n = run_case(c);
            if (n == 0) fail("a case the entry point declines, or one without a load", c);
            total += n;
        }
        printf("ok, %ld loads checked\n", total);
        return 0;
    }
    const int sizes[][2] = {{1, 1}, {1, 2}, {2, 3}, {3, 5}, {5, 7}, {7, 5}, {9, 13}, {14, 14}, {17, 9}, {28, 31}, {33, 29}};
    for (int R : {3, 5})
        for (int d : {2, 3, 4, 6, 12, 64})
            for (const auto& hw : sizes)
                for (int C : {1, 19, 100})
                    for (int N : {1, 3})
                        for (int pad : {0, 1, d * (R / 2), d * (R - 1)})
                            total += run_case(Case{R, d, N, hw[0], hw[1], C, pad, pad});
    total += run_case(Case{3, 2, 96, 112, 112, 32, 2, 2});      // more tiles than the launch has lanes: the stride over tiles
    total += run_case(Case{5, 12, 512, 14, 14, 320, 24, 24});
    printf("ok, %ld loads checked\n", total);
    return 0;
}
