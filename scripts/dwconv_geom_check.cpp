// Host check of the depthwise kernel's address arithmetic (csrc/fq_dwconv_i8_geom.h): every lane of every launch over the GPU
// tests' shapes loads inside the input, stores inside the output, and every output dword is written exactly once.
//   c++ -O2 -std=c++17 -o dwconv_geom_check scripts/dwconv_geom_check.cpp && ./dwconv_geom_check
//   ./dwconv_geom_check window=T R,stride,N,H,W,C,pad    a size-limit row instead of the built-in list: only the first and the last T
//                                                        tiles of the launch are walked, by the lanes and in the order the kernel visits
//                                                        them (neither tensor reaches 2^31 bytes: there is no boundary between); the
//                                                        32-bit tile, lane and offset arithmetic is checked against 64-bit arithmetic
// (tests/test_depthwise_plan_cpu.py runs it.)  The walk below is the kernel's own: same launch size, same lane -> (channel
// group, first tile, tile stride), same rows and columns per tile, the same predicates in front of every access.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_dwconv_i8_geom.h"

using namespace fq;

static void fail(const char* what, int R, int stride, int N, int H, int W, int C, int pad) {
    printf("%s: %dx%d stride %d, N %d, H %d, W %d, C %d, pad %d\n", what, R, R, stride, N, H, W, C, pad);
    exit(1);
}

static unsigned long g_window = 0;          // window=T: tiles [T, tiles - T) are skipped

template <int R, int STRIDE>
long run(int N, int H, int W, int C, int pad) {
    constexpr int TP = DwTile<R>::TP, NROWS = (TP - 1) * STRIDE + R, NPIX = (kDwTQ - 1) * STRIDE + R;
    if (H + 2 * pad < R || W + 2 * pad < R) return 0;
    const int Cpad = (C + 15) / 16 * 16;
    DwGeom g;
    g.N = N; g.H = H; g.W = W; g.Cpad = Cpad; g.C4 = Cpad / 4; g.pad_h = pad; g.pad_w = pad;
    g.P = (H + 2 * pad - R) / STRIDE + 1;
    g.Q = (W + 2 * pad - R) / STRIDE + 1;
    g.PB = (g.P + TP - 1) / TP;
    g.QB = (g.Q + kDwTQ - 1) / kDwTQ;
    g.tiles = (unsigned)((long)N * g.PB * g.QB);
    // the launch of dwconv_dispatch
    long blocks = ((long)g.tiles * g.C4 + kDwBlock - 1) / kDwBlock;
    if (blocks > kDwMaxBlocks) blocks = kDwMaxBlocks;
    const unsigned threads = (unsigned)blocks * kDwBlock, sp_stride = threads / g.C4;
    const size_t in_bytes = (size_t)N * H * W * Cpad, out_bytes = (size_t)N * g.P * g.Q * Cpad;
    if ((unsigned long)g.tiles + sp_stride > 0xffffffffUL || (unsigned long)g.tiles * g.C4 > 0xffffffffUL || in_bytes > 0xffffffffUL ||
        out_bytes > 0xffffffffUL)
        fail("32-bit tile or offset arithmetic wraps", R, STRIDE, N, H, W, C, pad);
    const bool windowed = g_window && (unsigned long)g.tiles > 2 * g_window;
    std::vector<bool> written(out_bytes / 4, false);
    long checked = 0;
    for (unsigned gid = 0; gid < threads; ++gid) {
        const int c4 = gid % g.C4;
        unsigned tile = gid / g.C4;
        if (tile >= sp_stride) continue;
        for (; tile < g.tiles; tile += sp_stride) {
            if (windowed && tile >= g_window && tile < g.tiles - g_window) {   // jump to this lane's first tile of the last window
                const unsigned long steps = ((unsigned long)(g.tiles - g_window) - tile + sp_stride - 1) / sp_stride;
                const unsigned long next = tile + steps * sp_stride;
                if (next >= g.tiles) break;
                tile = (unsigned)(next - sp_stride);
                continue;
            }
            const DwTilePos tp = dw_tile_pos<TP>(g, tile);
            if (tp.n < 0 || tp.n >= N) fail("image index out of range", R, STRIDE, N, H, W, C, pad);
            const int ih0 = tp.p0 * STRIDE - pad, iw0 = tp.q0 * STRIDE - pad;
            for (int i = 0; i < NROWS; ++i) {
                for (int k = 0; k < NPIX; ++k) {
                    if (!dw_in_ok(g, ih0 + i, iw0 + k)) continue;
                    if ((size_t)dw_in_off(g, tp.n, ih0 + i, iw0 + k, c4) + 4 > in_bytes) fail("load outside the input", R, STRIDE, N, H, W, C, pad);
                    if ((size_t)dw_in_off(g, tp.n, ih0 + i, iw0 + k, c4) != (((size_t)tp.n * H + (ih0 + i)) * W + (iw0 + k)) * Cpad + 4u * c4)
                        fail("input offset is not the pixel's", R, STRIDE, N, H, W, C, pad);
                    ++checked;
                }
            }
            for (int t = 0; t < TP; ++t) {
                for (int j = 0; j < kDwTQ; ++j) {
                    if (!dw_out_ok(g, tp.p0 + t, tp.q0 + j)) continue;
                    const unsigned o = dw_out_off(g, tp.n, tp.p0 + t, tp.q0 + j, c4);
                    if ((size_t)o + 4 > out_bytes || o % 4) fail("store outside the output", R, STRIDE, N, H, W, C, pad);
                    if ((size_t)o != (((size_t)tp.n * g.P + (tp.p0 + t)) * g.Q + (tp.q0 + j)) * Cpad + 4u * c4)
                        fail("output offset is not the pixel's", R, STRIDE, N, H, W, C, pad);
                    if (written[o / 4]) fail("output dword written twice", R, STRIDE, N, H, W, C, pad);
                    written[o / 4] = true;
                }
            }
        }
    }
    if (!windowed)
        for (bool v : written)
            if (!v) fail("output dword not written", R, STRIDE, N, H, W, C, pad);
    if (windowed) {                                       // every output of the whole images that the two windows cover
        const size_t img = (size_t)g.P * g.Q * Cpad / 4, imgs = g_window / ((size_t)g.PB * g.QB);
        if (imgs < 1) fail("window smaller than one image", R, STRIDE, N, H, W, C, pad);
        for (size_t i = 0; i < imgs * img; ++i)
            if (!written[i] || !written[written.size() - 1 - i]) fail("output dword of the first or last images not written", R, STRIDE, N, H, W, C, pad);
    }
    return checked;
}

int main(int argc, char** argv) {
    long total = 0;
    if (argc > 1) {
        for (int a = 1; a < argc; ++a) {
            int R, st, N, H, W, C, pad;
            if (strncmp(argv[a], "window=", 7) == 0) { g_window = strtoul(argv[a] + 7, nullptr, 10); continue; }
            if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d", &R, &st, &N, &H, &W, &C, &pad) != 7 || (R != 3 && R != 5) || (st != 1 && st != 2)) {
                printf("cannot read case %s\n", argv[a]);
                return 2;
            }
            total += R == 3 ? (st == 1 ? run<3, 1>(N, H, W, C, pad) : run<3, 2>(N, H, W, C, pad))
                            : (st == 1 ? run<5, 1>(N, H, W, C, pad) : run<5, 2>(N, H, W, C, pad));
        }
        printf("ok, %ld loads checked\n", total);
        return 0;
    }
    const int channels[] = {1, 16, 19, 32, 100, 256};
    const int sizes[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 3}, {3, 3}, {3, 5}, {5, 3}, {5, 6}, {5, 7}, {6, 11}, {7, 9}, {9, 13},
                            {13, 17}, {17, 9}, {28, 31}, {29, 41}, {33, 29}, {57, 55}, {112, 112}};
    for (int C : channels) {
        for (const auto& hw : sizes) {
            if ((long)C * hw[0] * hw[1] > 112L * 112 * 32) continue;
            for (int N : {1, 3}) {
                for (int pad : {0, 1, 2}) {
                    total += run<3, 1>(N, hw[0], hw[1], C, pad);
                    total += run<3, 2>(N, hw[0], hw[1], C, pad);
                }
                for (int pad : {0, 2, 4}) {
                    total += run<5, 1>(N, hw[0], hw[1], C, pad);
                    total += run<5, 2>(N, hw[0], hw[1], C, pad);
                }
            }
        }
    }
    total += run<3, 1>(64, 112, 112, 32, 1);          // more tiles than the launch has lanes: the stride over tiles
    total += run<5, 2>(256, 14, 14, 512, 2);
    printf("ok, %ld loads checked\n", total);
    return 0;
}
