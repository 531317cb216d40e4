// Host check of the re-quantising concat kernel (csrc/fq_concat_rq_i8_geom.h): every lane of every launch loads inside its source
// (aligned, a dword or 16 bytes), assembles exactly the elements the index rule asks for, every output chunk is written exactly
// once, an aligned launch is made of 16-byte loads only; the re-quantisation is v * 2^shift rounded half to even in double for
// all 256 int8 and all 65 536 int16 values, every shift in [-8, 8] and both ReLU flags, with every packed-int16 intermediate
// inside int16; the host guards answer the return codes of include/fq.h.
//   c++ -O2 -std=c++17 -fsanitize=address,undefined -o concat_rq_geom_check scripts/concat_rq_geom_check.cpp
//   ./concat_rq_geom_check                                            the built-in shape list
//   ./concat_rq_geom_check N,H,W/C0,C1,.../up0,.../bytes0,... ...      these cases instead; tests pass the GPU tests' and the models' lists
// One line per case: "case <text>: aligned16 A general G chunks X blocks B second-items S", then "requant: V values, T ties",
// "guards: G rows" and "ok, <loads> loads checked".  Exit status 1 at the first violation, 2 for a case that cannot be read.
// The walk is the kernel's own: same launch size, same lane -> (chunk, first pixel, stride), the same predicates in front of
// every load; bytes are carried through the same shift-and-mask steps on a model of memory whose every byte is its own address.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../pytorch-quantity_amd/csrc/fq_concat_rq_i8_geom.h"

using namespace fq;

struct Case { int N, H, W, nsrc, C[kCrqMaxSrc], up[kCrqMaxSrc], bytes[kCrqMaxSrc]; std::string text; };

static void fail(const char* what, const std::string& where) {
    printf("%s: %s\n", what, where.c_str());
    exit(1);
}

static std::string list_of(const int* v, int n) {
    std::string s;
    for (int i = 0; i < n; ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return s;
}

static std::string text_of(const Case& c) {
    return std::to_string(c.N) + "," + std::to_string(c.H) + "," + std::to_string(c.W) + "/" + list_of(c.C, c.nsrc) + "/" +
           list_of(c.up, c.nsrc) + "/" + list_of(c.bytes, c.nsrc);
}

// v_alignbyte_b32 on addresses: byte j of the result is byte sh + j of the pair {hi, lo}; -2 marks a byte that was not loaded
static void alignbyte(const long (&hi)[4], const long (&lo)[4], int sh, long (&out)[4]) {
    for (int j = 0; j < 4; ++j) out[j] = sh + j < 4 ? lo[sh + j] : hi[sh + j - 4];
}

static long run(const Case& c) {
    int Cpad[kCrqMaxSrc], relu[kCrqMaxSrc], shift[kCrqMaxSrc];
    long sum = 0;
    for (int i = 0; i < c.nsrc; ++i) {
        Cpad[i] = (c.C[i] + 15) / 16 * 16;
        relu[i] = i & 1;
        shift[i] = (i * 5) % 17 - 8;
        sum += c.C[i];
    }
    const int Cpad_out = (int)((sum + 15) / 16 * 16);
    if (crq_args(c.bytes, c.C, Cpad, c.up, relu, shift, c.nsrc, Cpad_out, c.N, c.H, c.W) != 0) fail("the guards refuse the case", c.text);
    const CrqGeom g = crq_geom(c.bytes, c.C, Cpad, c.up, relu, shift, c.nsrc, Cpad_out, c.N, c.H, c.W);
    long src_bytes[kCrqMaxSrc];
    for (int i = 0; i < kCrqMaxSrc; ++i)
        src_bytes[i] = i < c.nsrc ? (long)c.N * (c.H / c.up[i]) * (c.W / c.up[i]) * Cpad[i] * c.bytes[i] : 0;
    const bool general = !crq_aligned(g);
    const unsigned threads = (unsigned)crq_blocks(g) * kCatBlock, stride = threads / g.CH;
    if ((unsigned long)g.npix + stride > 0xffffffffUL || (unsigned long)g.npix * g.CH > 0xffffffffUL) fail("32-bit pixel arithmetic wraps", c.text);
    std::vector<unsigned char> written((size_t)g.npix * g.CH, 0);
    long loads = 0, second = 0;
    int n16 = 0, ngen = 0;
    for (unsigned gid = 0; gid < threads; ++gid) {
        const int k = gid % g.CH;
        unsigned pix = gid / g.CH;
        if (pix >= stride) continue;
        CrqPart part[kCrqMaxSrc];
        int owners = 0, whole = 0;
        for (int i = 0; i < kCrqMaxSrc; ++i) {
            part[i] = crq_part(g, k, i);
            owners += part[i].use;
            whole |= part[i].use & part[i].whole16;
        }
        const bool one16 = owners == 1 && whole;            // the kernel's test in front of crq_loop16
        if (!general && !one16) fail("aligned launch: the chunk is not 16 elements of one source", c.text);
        if (pix == 0) ++(one16 ? n16 : ngen);
        const unsigned first = pix;
        for (; pix < g.npix; pix += stride) {
            if (pix != first) ++second;
            const unsigned w = pix % g.W, h = (pix / g.W) % g.H, n = pix / g.W / g.H;
            long got[16];                                   // address of the element's first byte; -1: zero
            int got_src[16];
            for (int j = 0; j < 16; ++j) { got[j] = -1; got_src[j] = -1; }
            for (int i = 0; i < kCrqMaxSrc; ++i) {
                const CrqPart& p = part[i];
                if (!(i < g.nsrc) || !p.use) continue;
                if (!one16 && !p.ld) fail("a used part loads nothing", c.text);
                const int eb = g.s[i].wide ? 2 : 1;
                if (eb != c.bytes[i]) fail("element size", c.text);
                const unsigned sp = crq_src_pix(g, g.s[i].lu, n, h, w);
                if (g.s[i].lu == 0 && sp != pix) fail("source pixel of a source that is not upsampled", c.text);
                const long rowbytes = (long)g.s[i].Cpad * eb, row = (long)sp * rowbytes;
                long bytes[32];
                if (one16) {
                    for (int l = 0; l < eb; ++l) {
                        const long in_row = (long)p.s * eb + 16 * l, o = row + in_row;
                        if (o < 0 || o % 16 || o + 16 > src_bytes[i]) fail("16-byte load outside its source or unaligned", c.text);
                        if (in_row < 0 || in_row + 16 > rowbytes) fail("16-byte load outside its pixel row", c.text);
                        ++loads;
                        for (int j = 0; j < 16; ++j) bytes[16 * l + j] = o + j;
                    }
                } else {
                    long d[9][4];
                    for (int t = 0; t < 4 * eb + 1; ++t) {
                        for (int j = 0; j < 4; ++j) d[t][j] = -2;                   // not loaded: zero in the kernel
                        if (!(p.ld & (1u << t))) continue;
                        const long o = row + p.a + 4 * t;
                        if (o < 0 || o % 4 || o + 4 > src_bytes[i]) fail("dword load outside its source or unaligned", c.text);
                        if (p.a + 4 * t < 0 || p.a + 4 * t + 4 > rowbytes) fail("dword load outside its pixel row", c.text);
                        ++loads;
                        for (int j = 0; j < 4; ++j) d[t][j] = o + j;
                    }
                    if (p.ld >> (4 * eb + 1)) fail("a load bit past the part's dwords", c.text);
                    if (eb == 2 && (p.sh & 1)) fail("an int16 part at an odd byte", c.text);
                    for (int t = 0; t < 4 * eb; ++t) {
                        long o4[4];
                        alignbyte(d[t + 1], d[t], p.sh, o4);
                        for (int j = 0; j < 4; ++j) bytes[4 * t + j] = o4[j];
                    }
                }
                for (int t = 0; t < 4; ++t) {
                    const unsigned m = cat_dword_mask(one16 ? 0 : p.lo, p.hi, t);
                    for (int j = 0; j < 4; ++j) {
                        if (!((m >> (8 * j)) & 0xffu)) continue;
                        if (((m >> (8 * j)) & 0xffu) != 0xffu) fail("partial byte mask", c.text);
                        const int el = 4 * t + j;
                        if (got[el] != -1) fail("two sources write one output byte", c.text);
                        if (bytes[el * eb] < 0) fail("a wanted byte comes from a dword that was not loaded", c.text);
                        if (eb == 2 && (bytes[el * eb] % 2 || bytes[el * eb + 1] != bytes[el * eb] + 1)) fail("an int16 element is torn", c.text);
                        got[el] = bytes[el * eb];
                        got_src[el] = i;
                    }
                }
            }
            for (int j = 0; j < 16; ++j) {                  // the index rule and the channel mask
                const int ch = 16 * k + j;
                int i = -1;
                for (int q = 0; q < c.nsrc; ++q)
                    if (ch >= g.s[q].base && ch < g.s[q].base + c.C[q]) i = q;
                long want = -1;
                if (i >= 0) {
                    const int u = c.up[i];
                    want = ((((long)n * (c.H / u) + h / u) * (c.W / u) + w / u) * g.s[i].Cpad + (ch - g.s[i].base)) * c.bytes[i];
                }
                if (got[j] != want || got_src[j] != i) fail("output byte is not the element the index rule names", c.text);
            }
            if (((size_t)pix * g.CH + k + 1) * 16 > (size_t)g.npix * g.Cpad_out) fail("store outside the output", c.text);
            if (written[(size_t)pix * g.CH + k]++) fail("output chunk written twice", c.text);
        }
    }
    for (unsigned char v : written)
        if (v != 1) fail("output chunk not written", c.text);
    printf("case %s: aligned16 %d general %d chunks %lu blocks %ld second-items %ld\n", c.text.c_str(), n16, ngen,
           (unsigned long)g.npix * g.CH, crq_blocks(g), second);
    return loads;
}

static void check_requant() {
    long values = 0, ties = 0;
    for (int shift = -kCrqMaxShift; shift <= kCrqMaxShift; ++shift)
        for (int relu = 0; relu < 2; ++relu) {
            const CrqRound r = crq_round(shift, relu);
            const std::string where = "shift " + std::to_string(shift) + " relu " + std::to_string(relu);
            for (int v = -32768; v <= 32767; ++v) {
                const double exact = std::ldexp((double)v, shift);
                double want = std::nearbyint(exact);                           // round half to even (the default rounding mode)
                if (exact - std::floor(exact) == 0.5) ++ties;
                if (relu && want < 0) want = 0;
                want = want < -128 ? -128 : (want > 127 ? 127 : want);
                bool fits = false;
                if (crq_requant(v, r, &fits) != (int)want) fail("re-quantisation differs from rint(v * 2^shift)", where + " v " + std::to_string(v));
                if (!fits) fail("an intermediate leaves int16", where + " v " + std::to_string(v));
                ++values;
            }
        }
    printf("requant: %ld values (int8 is the range [-128, 127] of them), %ld ties\n", values, ties);
}

static void check_guards() {
    const int INV = -1, UNS = -4;
    struct Row { int want; int nsrc; int bytes[2], C[2], Cpad[2], up[2], relu[2], shift[2]; int Cpad_out, N, H, W; const char* what; };
    const Row rows[] = {
        {0, 2, {1, 2}, {16, 16}, {16, 16}, {1, 1}, {0, 1}, {-3, 2}, 32, 2, 4, 4, "a plain call"},
        {0, 1, {2, 0}, {16, 0}, {16, 0}, {1, 0}, {0, 0}, {0, 0}, 16, 1, 4, 4, "one int16 source at shift 0 is work"},
        {0, 1, {1, 0}, {16, 0}, {16, 0}, {1, 0}, {0, 0}, {1, 0}, 16, 1, 4, 4, "one int8 source at shift 1 is work"},
        {INV, 1, {1, 0}, {16, 0}, {16, 0}, {1, 0}, {0, 0}, {0, 0}, 16, 1, 4, 4, "nothing to do"},
        {INV, 0, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 0}, 32, 1, 4, 4, "no source"},
        {UNS, 9, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 0}, 32, 1, 4, 4, "nine sources"},
        {INV, 2, {1, 3}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 4, 4, "bytes 3"},
        {INV, 2, {0, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 4, 4, "bytes 0"},
        {INV, 2, {1, 1}, {0, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 16, 1, 4, 4, "C 0"},
        {INV, 2, {1, 1}, {17, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 48, 1, 4, 4, "Cpad < C"},
        {INV, 2, {1, 1}, {16, 16}, {16, 16}, {0, 1}, {0, 0}, {0, 1}, 32, 1, 4, 4, "up 0"},
        {INV, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {2, 0}, {0, 1}, 32, 1, 4, 4, "relu 2"},
        {INV, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 48, 1, 4, 4, "Cpad_out"},
        {INV, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, -1, 4, 4, "N < 0"},
        {INV, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 0, 4, "H 0"},
        {UNS, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 9}, 32, 1, 4, 4, "shift 9"},
        {UNS, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {-9, 0}, 32, 1, 4, 4, "shift -9"},
        {UNS, 2, {1, 1}, {16, 16}, {16, 16}, {3, 1}, {0, 0}, {0, 1}, 32, 1, 6, 6, "up 3"},
        {UNS, 2, {1, 1}, {16, 16}, {16, 16}, {2, 1}, {0, 0}, {0, 1}, 32, 1, 5, 4, "H % up"},
        {UNS, 2, {1, 1}, {16, 16}, {24, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 4, 4, "Cpad % 16"},
        {UNS, 2, {1, 1}, {65536, 16}, {65536, 16}, {1, 1}, {0, 0}, {0, 1}, 65552, 1, 4, 4, "sum C > 65536"},
        {0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 0, 1 << 30, 1 << 30, "N == 0"},
        {UNS, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 8192, 8192, "an output of 2^31 bytes"},
        {0, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 8192, 8191, "an output just under the limit"},
        {UNS, 2, {1, 2}, {1, 16}, {16, 1024}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 1024, 1024, "an int16 source of 2^31 bytes"},
        {0, 2, {1, 1}, {1, 16}, {16, 1024}, {1, 1}, {0, 0}, {0, 1}, 32, 1, 1024, 1024, "... that fits as int8"},
        {UNS, 2, {1, 1}, {16, 16}, {16, 16}, {1, 1}, {0, 0}, {0, 1}, 32, 1 << 30, 1 << 30, 1 << 30, "sizes whose product leaves long"},
    };
    int n = 0;
    for (const Row& r : rows) {
        if (crq_args(r.bytes, r.C, r.Cpad, r.up, r.relu, r.shift, r.nsrc, r.Cpad_out, r.N, r.H, r.W) != r.want) fail("guard", r.what);
        ++n;
    }
    const int C[2] = {16, 16}, up[2] = {1, 4}, by[2] = {1, 2}, sh[2] = {-8, 8}, sh9[2] = {0, 9}, by3[2] = {1, 3};
    if (!crq_supported(C, up, by, sh, 2) || crq_supported(C, up, by, sh9, 2) || crq_supported(C, up, by3, sh, 2) ||
        crq_supported(C, up, by, sh, 0) || crq_supported(nullptr, up, by, sh, 2))
        fail("guard", "crq_supported");
    printf("guards: %d rows\n", n + 5);
}

static bool parse_list(const std::string& s, int* out, int& n) {
    n = 0;
    const char* p = s.c_str();
    while (*p) {
        char* end;
        const long v = strtol(p, &end, 10);
        if (end == p || n >= kCrqMaxSrc || (*end && *end != ',')) return false;
        out[n++] = (int)v;
        p = *end == ',' ? end + 1 : end;
    }
    return n > 0;
}

static bool parse(const char* arg, Case& c) {
    std::vector<std::string> parts;
    std::string a(arg);
    size_t at = 0;
    for (;;) {
        const size_t p = a.find('/', at);
        parts.push_back(a.substr(at, p == std::string::npos ? p : p - at));
        if (p == std::string::npos) break;
        at = p + 1;
    }
    if (parts.size() != 4 || sscanf(parts[0].c_str(), "%d,%d,%d", &c.N, &c.H, &c.W) != 3) return false;
    int nc = 0, nu = 0, nb = 0;
    if (!parse_list(parts[1], c.C, nc) || !parse_list(parts[2], c.up, nu) || !parse_list(parts[3], c.bytes, nb) || nc != nu || nc != nb)
        return false;
    c.nsrc = nc;
    c.text = text_of(c);
    return c.N > 0 && c.H > 0 && c.W > 0;
}

static Case make(int N, int H, int W, std::vector<int> C, std::vector<int> up, std::vector<int> bytes) {
    Case c;
    c.N = N; c.H = H; c.W = W; c.nsrc = (int)C.size();
    for (int i = 0; i < c.nsrc; ++i) {
        c.C[i] = C[i];
        c.up[i] = i < (int)up.size() ? up[i] : 1;
        c.bytes[i] = i < (int)bytes.size() ? bytes[i] : 1;
    }
    c.text = text_of(c);
    return c;
}

int main(int argc, char** argv) {
    std::vector<Case> cases;
    for (int a = 1; a < argc; ++a) {
        Case c;
        if (!parse(argv[a], c)) {
            printf("cannot read case %s\n", argv[a]);
            return 2;
        }
        cases.push_back(c);
    }
    if (cases.empty()) {
        const int planes[][3] = {{1, 1, 1}, {1, 2, 2}, {3, 4, 12}, {2, 8, 8}};
        const std::vector<std::vector<int>> chans = {{16}, {3}, {16, 16}, {64, 64}, {1, 3}, {19, 33}, {100, 16, 1}, {33, 19, 3},
                                                     {16, 32, 48}, {1, 3, 16, 19, 33, 100, 1, 3}, {16, 16, 16, 16, 16, 16, 16, 16}};
        const std::vector<std::vector<int>> sizes = {{1, 1, 1, 1, 1, 1, 1, 1}, {2, 2, 2, 2, 2, 2, 2, 2}, {1, 2, 1, 2, 2, 1, 2, 1},
                                                     {2, 1, 2, 1, 1, 2, 1, 2}};
        const std::vector<std::vector<int>> factors = {{1, 1, 1, 1, 1, 1, 1, 1}, {2, 1, 4, 1, 2, 1, 4, 1}, {4, 2, 1, 4, 1, 2, 1, 4}};
        for (const auto& ch : chans)
            for (const auto& pl : planes)
                for (const auto& by : sizes)
                    for (const auto& f : factors) {
                        bool ok = true;
                        for (size_t i = 0; i < ch.size(); ++i) ok = ok && pl[1] % f[i] == 0 && pl[2] % f[i] == 0;
                        if (ok) cases.push_back(make(pl[0], pl[1], pl[2], ch, f, by));
                    }
        cases.push_back(make(3, 120, 120, {100, 100}, {1, 2}, {2, 1}));     // more chunks than the launch has lanes: the stride over pixels
        cases.push_back(make(9, 64, 64, {64, 64, 64, 64}, {}, {2, 1, 1, 2}));
    }
    long total = 0;
    for (const Case& c : cases) total += run(c);
    check_requant();
    check_guards();
    printf("ok, %ld loads checked\n", total);
    return 0;
}
