// Host check of the atrous dense fp32 kernel's address arithmetic (csrc/fq_conv_dil_f32_geom.h): over the shapes given and
// the dilated layers of model/deeplab/DeepLabV3_fabu.py at both output strides, for every tile of every launch (the plain grid
// and the histogram form's smaller one): every staged element comes from inside x and from the tile's image, every LDS read lies
// in the staged pixels or the zero pixel, every live tap reads the float staged from its pixel (or the zero pixel where that
// pixel lies outside the image), every culled tap is dead for every pixel of its tile, and every output is written exactly once.
//   c++ -O2 -std=c++17 -fsanitize=address,undefined -o conv_dil_f32_geom_check scripts/conv_dil_f32_geom_check.cpp
//   ./conv_dil_f32_geom_check                                    the model's layers and the sweep below
//   ./conv_dil_f32_geom_check N,Cin,Cout,H,W,d,pad ...           these shapes instead
// (tests/test_conv_dil_f32_cpu.py runs it both ways, the second with the GPU tests' shapes of tests/conv_dil_f32_cases.py.)  The walk below is the kernel's own: same plan, same grid, same workgroup -> tiles,
// same lane -> pixel, the same predicates in front of every access.  One chunk of channels is walked per tile: the chunk only
// adds (c0 + c) H W to a staged element's offset, and the largest such offset is checked.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_conv_dil_f32_geom.h"

using namespace fq;

struct Shape { int N, Cin, Cout, H, W, d, pad; };

static void fail(const char* what, const Shape& s) {
    printf("%s: N %d, Cin %d, Cout %d, H %d, W %d, dilation %d, pad %d\n", what, s.N, s.Cin, s.Cout, s.H, s.W, s.d, s.pad);
    exit(1);
}

static long run(const Shape& s, bool hist, long* live_taps, long* tiles) {
    CdGeom g;
    if (!cd_plan(g, s.N, s.Cin, s.Cout, s.H, s.W, s.d, s.pad)) fail("the plan declines a shape of the list", s);
    const size_t plane = (size_t)s.H * s.W, in_elems = (size_t)s.N * s.Cin * plane, out_elems = (size_t)s.N * s.Cout * g.Ho * g.Wo;
    if (in_elems >= (1ul << 30) || out_elems >= (1ul << 30) || 9ul * s.Cin * s.Cout >= (1ul << 30)) fail("32-bit offset arithmetic wraps", s);
    if (g.TH < 1 || g.TW < 1 || g.TW > kCdMaxTW || g.TH * g.TW > kCdTilePx || (g.MT != 1 && g.MT != 2) || g.RB * g.TH < g.Ho ||
        g.CB * g.TW < g.Wo || g.MB * 32 * g.MT < s.Cout || s.Cin % kCdChunk || kCdPxPerThread * kCdBlock < kCdMaxPx)
        fail("tiles that do not cover the layer", s);
    bool rows[32] = {false};
    for (int e = 0; e < 16; ++e)
        for (unsigned h = 0; h < 2; ++h) {
            const unsigned r = cd_acc_row(e, h);
            if (r >= 32 || rows[r]) fail("accumulator rows are no permutation", s);
            rows[r] = true;
        }
    const size_t lds = (size_t)kCdZero + (size_t)kCdMaxPx * kCdPitch;
    std::vector<unsigned char> written(out_elems, 0);
    std::vector<long> src(kCdMaxPx, -1);                  // what each staged pixel holds: ih W + iw
    const unsigned G = cd_grid(g, hist);
    long loads = 0;
    for (unsigned b = 0; b < G; ++b) {
        for (unsigned tile = geom_first_tile(b, G); tile < g.tiles; tile += G) {
            const CdTilePos tp = cd_tile_pos(g, tile);
            if (tp.n >= (unsigned)s.N || tp.m0 >= (unsigned)s.Cout || tp.p0 >= g.Ho || tp.q0 >= g.Wo || tp.th < 1 || tp.tw < 1)
                fail("tile outside the tensor", s);
            if (tp.staged > (unsigned)kCdMaxPx || tp.staged < 1) fail("more staged pixels than the LDS holds, or none", s);
            for (unsigned px = 0; px < tp.staged; ++px) { // (thread px % 256, its pixel px / 256)
                const unsigned off = cd_stage_src(g, tp, px);
                if (off >= plane) fail("staged element outside its plane", s);
                if ((size_t)cd_x_plane(g, tp.n, (unsigned)s.Cin - 1u) + off >= in_elems) fail("staged element outside the input", s);
                if (cd_x_plane(g, tp.n, 0) / (s.Cin * plane) != tp.n) fail("staged element of another image", s);
                src[px] = (long)off;
                ++loads;
            }
            for (int t = 0; t < 9; ++t)
                if ((tp.rows.live >> (t / 3)) & (tp.cols.live >> (t % 3)) & 1) ++*live_taps;
            ++*tiles;
            for (unsigned j = 0; j < (unsigned)kCdTilePx; ++j) {
                CdLanePos lp;
                const bool has = cd_lane_pos(g, tp, j, &lp);
                if (has && !cd_wave_active(g, tp, j / 32u)) fail("a wave with a pixel skips the K loop", s);
                for (int r = 0; r < 3; ++r) {
                    for (int c = 0; c < 3; ++c) {
                        const unsigned rd = cd_read_index(g, tp, has, lp, r, c);
                        const bool live = ((tp.rows.live >> r) & (tp.cols.live >> c) & 1) != 0;
                        const long ih = (long)lp.p - s.pad + (long)r * s.d, iw = (long)lp.q - s.pad + (long)c * s.d;
                        const bool in = has && ih >= 0 && ih < s.H && iw >= 0 && iw < s.W;
                        if (!live) {
                            if (in) fail("a culled tap has a source pixel inside the image", s);
                            continue;                         // (the kernel never reads for it)
                        }
                        if ((size_t)rd + 1 + kCdChunk > lds) fail("LDS read outside the staged pixels and the zero pixel", s);
                        if (!in) {
                            if (rd != 0) fail("a tap outside the image does not read the zero pixel", s);
                            continue;
                        }
                        if (rd < (unsigned)kCdZero || (rd - kCdZero) % kCdPitch) fail("LDS read between staged pixels", s);
                        const unsigned px = (rd - kCdZero) / kCdPitch;
                        if (px >= tp.staged || src[px] != ih * s.W + iw) fail("a tap reads another pixel's LDS floats", s);
                    }
                }
                if (!has) continue;
                for (int mt = 0; mt < g.MT; ++mt)
                    for (int e = 0; e < 16; ++e)
                        for (unsigned h = 0; h < 2; ++h) {
                            const unsigned k = tp.m0 + (unsigned)mt * 32u + cd_acc_row(e, h);
                            if (k >= (unsigned)s.Cout) continue;
                            const unsigned o = cd_out_off(g, tp.n, k, lp);
                            if ((size_t)o >= out_elems) fail("store outside the output", s);
                            if ((long)o != (((long)tp.n * s.Cout + k) * g.Ho + lp.p) * g.Wo + lp.q) fail("store to the wrong element", s);
                            if (written[o]++) fail("output element written twice", s);
                        }
            }
        }
    }
    for (unsigned char v : written)
        if (v != 1) fail("output element not written", s);
    return loads;
}

int main(int argc, char** argv) {
    long total = 0, live = 0, tiles = 0;
    if (argc > 1) {
        for (int a = 1; a < argc; ++a) {
            Shape s;
            if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d", &s.N, &s.Cin, &s.Cout, &s.H, &s.W, &s.d, &s.pad) != 7) {
                printf("cannot read case %s\n", argv[a]);
                return 2;
            }
            live = tiles = 0;
            total += run(s, true, &live, &tiles);
            live = tiles = 0;
            total += run(s, false, &live, &tiles);
            printf("%s: %ld tiles, %.2f live taps per tile\n", argv[a], tiles, (double)live / (double)tiles);
        }
        printf("ok, %ld loads\n", total);
        return 0;
    }
    // the dilated dense layers of DeepLabV3_fabu at 224 x 224, width 64, two images: output stride 16 (layer4 at d = 2 on 14 x 14,
    // ASPP 2048 -> 256 at 6 / 12 / 18) and output stride 8 (layer3 at 2, layer4 at 2 and 4 on 28 x 28, ASPP at 12 / 24 / 36); the
    // narrow model of the GPU test (width 16 on 64 x 64: 4 x 4 planes); then the largest dilation with the largest padding, a
    // plane of one output, and a plane higher than wide
    const Shape net[] = {{2, 512, 512, 14, 14, 2, 2},   {2, 2048, 256, 14, 14, 6, 6},   {2, 2048, 256, 14, 14, 12, 12},
                         {2, 2048, 256, 14, 14, 18, 18}, {2, 256, 256, 28, 28, 2, 2},    {2, 512, 512, 28, 28, 2, 2},
                         {2, 512, 512, 28, 28, 4, 4},    {2, 2048, 256, 28, 28, 12, 12}, {2, 2048, 256, 28, 28, 24, 24},
                         {2, 2048, 256, 28, 28, 36, 36}, {2, 128, 128, 4, 4, 2, 2},      {2, 512, 64, 4, 4, 18, 18},
                         {1, 16, 4, 70, 90, 64, 128},    {1, 16, 4, 5, 7, 2, 0},         {1, 16, 4, 129, 1, 64, 64},
                         {3, 16, 36, 200, 9, 7, 7}};
    for (const Shape& s : net)
        for (bool hist : {false, true}) total += run(s, hist, &live, &tiles);
    // every padding at an odd size
    for (int d : {2, 3, 5})
        for (int pad = 0; pad <= 2 * d; ++pad)
            if (21 + 2 * pad >= 2 * d + 1) total += run({2, 16, 12, 21, 23, d, pad}, false, &live, &tiles);
    printf("ok, %ld loads\n", total);
    return 0;
}
