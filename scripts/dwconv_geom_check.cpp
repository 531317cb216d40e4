// Host check of the depthwise kernel's address arithmetic (csrc/fq_dwconv_i8_geom.h): every lane of every launch over the GPU
// tests' shapes loads inside the input, stores inside the output, and every output dword is written exactly once.
//   c++ -O2 -std=c++17 -o dwconv_geom_check scripts/dwconv_geom_check.cpp && ./dwconv_geom_check
// (tests/test_depthwise_plan_cpu.py runs it.)  The walk below is the kernel's own: same launch size, same lane -> (channel
// group, first tile, tile stride), same rows and columns per tile, the same predicates in front of every access.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_dwconv_i8_geom.h"

using namespace fq;

static void fail(const char* what, int R, int stride, int N, int H, int W, int C, int pad) {
    printf("%s: %dx%d stride %d, N %d, H %d, W %d, C %d, pad %d\n", what, R, R, stride, N, H, W, C, pad);
    exit(1);
}

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
    std::vector<unsigned char> written(out_bytes / 4, 0);
    long checked = 0;
    for (unsigned gid = 0; gid < threads; ++gid) {
        const int c4 = gid % g.C4;
        unsigned tile = gid / g.C4;
        if (tile >= sp_stride) continue;
        for (; tile < g.tiles; tile += sp_stride) {
            const DwTilePos tp = dw_tile_pos<TP>(g, tile);
            if (tp.n < 0 || tp.n >= N) fail("image index out of range", R, STRIDE, N, H, W, C, pad);
            const int ih0 = tp.p0 * STRIDE - pad, iw0 = tp.q0 * STRIDE - pad;
            for (int i = 0; i < NROWS; ++i) {
                for (int k = 0; k < NPIX; ++k) {
                    if (!dw_in_ok(g, ih0 + i, iw0 + k)) continue;
                    if ((size_t)dw_in_off(g, tp.n, ih0 + i, iw0 + k, c4) + 4 > in_bytes) fail("load outside the input", R, STRIDE, N, H, W, C, pad);
                    ++checked;
                }
            }
            for (int t = 0; t < TP; ++t) {
                for (int j = 0; j < kDwTQ; ++j) {
                    if (!dw_out_ok(g, tp.p0 + t, tp.q0 + j)) continue;
                    const unsigned o = dw_out_off(g, tp.n, tp.p0 + t, tp.q0 + j, c4);
                    if ((size_t)o + 4 > out_bytes || o % 4) fail("store outside the output", R, STRIDE, N, H, W, C, pad);
                    if (written[o / 4]++) fail("output dword written twice", R, STRIDE, N, H, W, C, pad);
                }
            }
        }
    }
    for (unsigned char v : written)
        if (v != 1) fail("output dword not written", R, STRIDE, N, H, W, C, pad);
    return checked;
}

int main() {
    long total = 0;
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
