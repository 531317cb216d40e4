// Host check of the dense int8 convolution's kernel choice (csrc/fq_conv_i8_select.h): prints the whole ConvChoice of every case
// and asserts what must hold of any choice, on a box without a GPU.
//   g++ -O2 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o conv_i8_select_check scripts/conv_i8_select_check.cpp
//   ./conv_i8_select_check [NAME=value ...] N,H,W,C,K,R,S,sh,sw,ph,pw,dh,dw/outs[/pcs] ...
// NAME=value: an FQ_* switch as the environment would hold it (NAME= is the empty string); they go through the library's own
// parse function, the getter reads argv instead of the environment.  outs: y (fp32 NCHW), q (int8 NHWC), yq (both), add (the
// fused residual add); /pcs: one shift per output channel.
// One line per case:
//   case <text>: <variant>/<tk> family F path P stages S np NP out O grid X,Y block B lds L xcd_kt A tiles_m T slab R pixels X
//   tiles T chunk C | refused: <variant>/<tk>
// (`refused`: what the dispatcher falls to when the runtime refuses the dynamic LDS of the halo families -- a path no test can
// take on a GPU.)  Then "ok, <n> cases".  Exit status 1 at the first violated invariant, 2 for an argument it cannot read.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_conv_i8_select.h"

using namespace fq::sel;

struct Geom {                            // the geometry fields of ConvParams
    int N, H, W, C, K, R, S, P, Q, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, M, chunks;
};
struct Case { Geom g; ConvOuts o; std::string text; };

static std::vector<std::string> g_switches;     // NAME=value
static const char* switch_value(const char* name) {
    const size_t n = strlen(name);
    for (const std::string& s : g_switches)
        if (s.size() > n && s.compare(0, n, name) == 0 && s[n] == '=') return s.c_str() + n + 1;
    return nullptr;
}

static const char* variant_name(int v) {
    switch (v) {
        case kVarC64Halo: return "c64_halo";
        case kVarHalo8: return "halo8";
        case kVarHalo: return "halo";
        case kVarDma2: return "dma2";
        case kVarDma3: return "dma3";
        case kVarTileC128: return "tile_c128";
        case kVarTileC64: return "tile_c64";
        case kVarTileGeneral: return "tile_general";
        case kVarLinearWave: return "linear_wave";
    }
    return "?";
}

static void fail(const char* what, const Case& c) {
    printf("%s: %s\n", what, c.text.c_str());
    exit(1);
}
#define NEED(cond, what) do { if (!(cond)) fail(what, cs); } while (0)

static long ceil_div(long a, long b) { return (a + b - 1) / b; }

static void check(const Case& cs, const ConvChoice& c, const ConvSwitches& sw, unsigned excluded) {
    const Geom& g = cs.g;
    const ConvOuts& o = cs.o;
    NEED(!(c.family & excluded), "an excluded family was chosen");
    const int want_out = (o.res ? kOutI8 | kOutAdd : (o.y && o.q ? kOutF32 | kOutI8 : (o.q ? kOutI8 : kOutF32))) | (o.pcs ? kOutPcs : 0);
    NEED(c.out == want_out, "output bits");
    NEED(!(c.out & kOutAdd) || c.family == kFamDma || c.family == kFamTile, "the fused add outside the register-staged and LDS-DMA kernels");
    NEED(c.grid_x >= 1 && c.grid_x < 0x7fffffffu && c.grid_y >= 1 && c.grid_y <= 65535, "grid outside the launch limits");
    if (c.family == kFamLinear) {
        NEED(c.variant == kVarLinearWave && c.tk == 32 && c.block == 64 * kLinWaves && c.lds == 0, "linear_wave fields");
        NEED(g.H == 1 && g.W == 1 && g.R == 1 && g.S == 1 && g.P == 1 && g.Q == 1 && g.pad_h == 0 && g.pad_w == 0 && g.dil_h == 1 &&
             g.dil_w == 1 && o.y && !o.q && !o.res, "linear_wave off the 1x1 plane with pad 0, dilation 1 and an fp32 output alone");
        NEED(c.grid_x == (unsigned)ceil_div(g.K, 32) && c.grid_y == (unsigned)ceil_div(g.M, 32), "linear_wave grid");
        return;
    }
    const bool halo3x3 = g.R == 3 && g.S == 3 && g.stride_h == 1 && g.stride_w == 1 && g.pad_h == 1 && g.pad_w == 1 && g.dil_h == 1 &&
                         g.dil_w == 1 && !o.res;
    if (c.family == kFamC64Halo) {
        NEED(c.variant == kVarC64Halo && c.tk == 64 && c.block == kConvBlock, "c64_halo fields");
        NEED(halo3x3 && g.C == 64 && g.K <= 64, "c64_halo off its shape");
        NEED(c.lds <= two_per_cu_lds(64, o.pcs), "c64_halo does not fit two workgroups per CU");
        NEED(c.slab_rows >= 130 + 2 * g.W && c.slab_rows % 16 == 0 && c.total_pixels == g.N * g.H * g.W, "c64_halo slab");
        NEED(c.lds == 9u * 64 * 64 + 64 * 8 + 64 + kTP * 80 + 2u * c.slab_rows * 64, "c64_halo LDS bytes");
        NEED(c.tiles == ceil_div(g.M, kTP) && c.tiles_m == c.tiles && c.xcd_kt == 0, "c64_halo tiles");
        NEED(c.xcd_chunk == (sw.c64_xcd ? (int)ceil_div(c.tiles, 8) : 0), "c64_halo XCD chunk");
        // persistent: the workgroups walk the tiles; at least one, never more than there are tiles
        NEED(c.grid_y == 1 && (long)c.grid_x <= c.tiles && (long)c.grid_x <= (long)kCUs * sw.c64_wg_per_cu, "c64_halo grid");
        return;
    }
    NEED(c.tk == 64 || c.tk == 128, "tile height");
    long tile = kTP;
    if (c.family == kFamHalo) {
        NEED(c.variant == kVarHalo8 || c.variant == kVarHalo, "halo variant");
        NEED(halo3x3, "a halo kernel off the 3x3 / stride 1 / pad 1 shape");
        NEED(c.np == 1 || (c.np == 2 && c.variant == kVarHalo), "halo sub-tiles");
        tile = c.variant == kVarHalo8 ? 256 : 128 * c.np;
        NEED(c.block == (unsigned)(c.variant == kVarHalo8 ? 2 * kConvBlock : kConvBlock), "halo block");
        NEED(c.lds <= two_per_cu_lds(c.tk, o.pcs), "a halo kernel does not fit two workgroups per CU");
        NEED(c.slab_rows >= tile + 2 + 2 * g.W && c.slab_rows % 8 == 0 && c.total_pixels == g.N * g.H * g.W, "halo slab");
        NEED(c.lds == (unsigned)c.stages * c.tk * 128 + c.tk * 8 + 128 + (unsigned)c.slab_rows * 128, "halo LDS bytes");
    } else {
        NEED(c.block == kConvBlock && c.lds == 0, "block / LDS of a kernel without dynamic LDS");
        if (c.family == kFamDma) NEED(c.variant == (c.stages == 3 ? kVarDma3 : kVarDma2), "dma variant");
        else NEED(c.family == kFamTile && c.variant == (c.path == kPathC128 ? kVarTileC128 : (c.path == kPathC64 ? kVarTileC64 : kVarTileGeneral)), "tile variant");
        if (c.family == kFamTile && c.path == kPathC64) NEED(g.C == 64, "tile_c64 with C != 64");
    }
    if (c.family != kFamTile) NEED(c.stages == 2 || c.stages == 3, "ring depth");
    if (c.family != kFamTile || c.path == kPathC128) NEED(g.C % 128 == 0 && g.K % c.tk == 0, "C % 128 or K % TK");
    // the grid covers ceil(M / tile) x ceil(K / TK) tiles, plain or in the XCD-aware order
    const long gx = ceil_div(g.M, tile), gy = ceil_div(g.K, c.tk);
    NEED(c.tiles_m == gx, "tiles_m");
    const long padded = ceil_div(gx, 8) * 8 * gy;
    if (sw.xcd && gy > 1 && padded < 0x7fffffffL) {
        NEED(c.xcd_kt == gy && c.grid_x == padded && c.grid_y == 1, "XCD-ordered grid");
    } else {
        NEED(c.xcd_kt == 0 && c.grid_x == gx && c.grid_y == gy, "plain grid");
    }
}

static void print_choice(const ConvChoice& c) {
    printf("%s/%d family %u path %d stages %d np %d out %d grid %u,%u block %u lds %u xcd_kt %d tiles_m %d slab %d pixels %d tiles %d chunk %d",
           variant_name(c.variant), c.tk, c.family, c.path, c.stages, c.np, c.out, c.grid_x, c.grid_y, c.block, c.lds, c.xcd_kt,
           c.tiles_m, c.slab_rows, c.total_pixels, c.tiles, c.xcd_chunk);
}

static bool parse(const char* arg, Case& c) {
    const std::string a(arg);
    const size_t p1 = a.find('/');
    if (p1 == std::string::npos) return false;
    const size_t p2 = a.find('/', p1 + 1);
    Geom& g = c.g;
    char extra;
    if (sscanf(a.substr(0, p1).c_str(), "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d%c", &g.N, &g.H, &g.W, &g.C, &g.K, &g.R, &g.S, &g.stride_h,
               &g.stride_w, &g.pad_h, &g.pad_w, &g.dil_h, &g.dil_w, &extra) != 13)
        return false;
    const std::string outs = a.substr(p1 + 1, p2 == std::string::npos ? std::string::npos : p2 - p1 - 1);
    c.o = ConvOuts{outs == "y" || outs == "yq", outs == "q" || outs == "yq", outs == "add", false};
    if (!c.o.y && !c.o.q && !c.o.res) return false;
    if (p2 != std::string::npos) {
        if (a.substr(p2 + 1) != "pcs") return false;
        c.o.pcs = true;
    }
    // what conv2d_i8_dispatch refuses before it selects
    if (g.N <= 0 || g.H <= 0 || g.W <= 0 || g.C <= 0 || g.K <= 0 || g.R <= 0 || g.S <= 0 || g.stride_h <= 0 || g.stride_w <= 0 ||
        g.pad_h < 0 || g.pad_w < 0 || g.dil_h <= 0 || g.dil_w <= 0 || g.C % 16)
        return false;
    g.P = (g.H + 2 * g.pad_h - g.dil_h * (g.R - 1) - 1) / g.stride_h + 1;
    g.Q = (g.W + 2 * g.pad_w - g.dil_w * (g.S - 1) - 1) / g.stride_w + 1;
    const long M = (long)g.N * g.P * g.Q;
    if (g.P <= 0 || g.Q <= 0 || M > 0x7fffffffL || (long)g.N * g.H * g.W * g.C >= 0x7fffffffL || (long)g.K * g.R * g.S * g.C >= 0x7fffffffL ||
        (long)g.K * g.P * g.Q > 0x1fffffffL)
        return false;
    g.M = (int)M;
    g.chunks = g.R * g.S * (g.C / 16);
    c.text = a;
    return true;
}

int main(int argc, char** argv) {
    std::vector<Case> cases;
    for (int a = 1; a < argc; ++a) {
        if (strncmp(argv[a], "FQ_", 3) == 0 && strchr(argv[a], '=')) { g_switches.push_back(argv[a]); continue; }
        Case c;
        if (!parse(argv[a], c)) {
            printf("cannot read case %s\n", argv[a]);
            return 2;
        }
        cases.push_back(c);
    }
    const ConvSwitches sw = read_conv_switches(switch_value);
    printf("switches: xcd %d stages %d halo %d halo_stages %d halo_np %d halo8 %d c64_halo %d c64_xcd %d c64_wg_per_cu %d linear_wave %d "
           "dma %d tk %d c64 %d\n", sw.xcd, sw.stages, sw.halo, sw.halo_stages, sw.halo_np, sw.halo8, sw.c64_halo, sw.c64_xcd,
           sw.c64_wg_per_cu, sw.linear_wave, sw.dma, sw.tk, sw.c64);
    for (const Case& cs : cases) {
        const ConvChoice c = select_conv_i8(cs.g, cs.o, sw);
        check(cs, c, sw, 0);
        printf("case %s: ", cs.text.c_str());
        print_choice(c);
        if (c.family == kFamC64Halo || c.family == kFamHalo) {
            const ConvChoice next = select_conv_i8(cs.g, cs.o, sw, c.family);
            check(cs, next, sw, c.family);
            printf(" | refused: %s/%d", variant_name(next.variant), next.tk);
        }
        printf("\n");
    }
    printf("ok, %zu cases\n", cases.size());
    return 0;
}
