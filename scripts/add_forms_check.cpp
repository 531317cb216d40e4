// Host check of the resident NewAdd's form selection (csrc/fq_add_params.h) and of each form's range argument.
//   g++ -O2 -std=c++20 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o add_forms_check
//       scripts/add_forms_check.cpp && ./add_forms_check
// (tests/test_add_rule_cpu.py runs it.)  The three forms of add_resident_16_regs (csrc/fq_resident.h) are written out below in
// plain C++ AS THE KERNELS COMPUTE THEM, one element at a time: the packed form with explicit 16-bit wrap-around and a
// saturating add, the 32-bit form in int32_t (the sanitizer turns an overflow into a failure), the chain in float.  For EVERY
// (gx, gy, ib) in [-16, 16]^3, ReLU on and off and all four operand-type pairs -- 287 496 parameter sets -- and over the boundary
// operand set of tests/add_rule.py (boundary_pairs, rebuilt here), it runs
//   * the form make_add_params selects (add_resident_form), after checking that the form's STATED precondition holds there, and
//   * every other form whose stated precondition holds,
// against the rule of include/fq.h transcribed in int64_t.  It says nothing about the compiled kernels; it says that the
// selection never picks a form outside its proof, and that each proof's range argument holds on these operands.
//   ./add_forms_check pairs xb yb gx gy ib     prints the operand set of one parameter set (held against the Python one)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "../pytorch-quantity_amd/csrc/fq_add_params.h"
using namespace fq;

// ---- the rule, int64 (tests/add_rule.py) ----------------------------------------------------------------------------------
static const int64_t kLo = -128 * (int64_t(1) << 16), kHi = 127 * (int64_t(1) << 16);
static int64_t pow2(int n) { return int64_t(1) << n; }
static int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int64_t floor_div_pow2(int64_t v, int sh) { return v >> sh; }                   // arithmetic: defined since C++20
static int64_t rule_sum(int x, int y, int gx, int gy, int relu) {
    return clamp64(x * pow2(16 - gx) + y * pow2(16 - gy), relu ? 0 : kLo, kHi);
}
static int rule_narrow(int64_t S, int ib) {
    const int sh = 16 - ib;
    int64_t q = S;
    if (sh > 0) {
        const int64_t fl = floor_div_pow2(S, sh), rem = S - fl * pow2(sh), half = pow2(sh - 1);
        q = fl + ((rem > half || (rem == half && (fl & 1))) ? 1 : 0);
    }
    return (int)clamp64(q, -128, 127);
}

// ---- the boundary operand set (tests/add_rule.py: BASE8, BASE16, TIES, DELTAS, targets, boundary_pairs) --------------------
static const int kBase8[] = {-128, -127, -1, 0, 1, 126, 127};
static const int kBase16[] = {-128, -127, -1, 0, 1, 126, 127, -32768, -32767, -129, 128, 32766, 32767};
static const int kTies[] = {-129, -128, -2, -1, 0, 1, 126, 127};
typedef std::vector<std::pair<int, int>> Pairs;

static void solve(const std::vector<int>& fixed, int g_fixed, int g_free, int free_bytes, const std::vector<int64_t>& T, bool fixed_is_x,
                  Pairs& out) {
    const int sh = 16 - g_free, lim = free_bytes == 1 ? 128 : 32768;
    for (int64_t t : T)
        for (int f : fixed) {
            const int64_t need = t - f * pow2(16 - g_fixed);
            const int64_t q = floor_div_pow2(need, sh);
            if (need - q * pow2(sh) != 0) continue;
            for (int d = -1; d <= 1; ++d) {
                const int64_t v = q + d;
                if (v < -lim || v >= lim) continue;
                out.push_back(fixed_is_x ? std::make_pair(f, (int)v) : std::make_pair((int)v, f));
            }
        }
}

static void boundary_pairs(int xb, int yb, int gx, int gy, int ib, Pairs& out) {
    out.clear();
    std::vector<int> bx(kBase16, kBase16 + (xb == 1 ? 7 : 13)), by(kBase16, kBase16 + (yb == 1 ? 7 : 13));
    (void)kBase8;                                                                       // (the first seven of kBase16)
    std::vector<int64_t> T = {kLo, 0, kHi};
    if (ib < 16) for (int v : kTies) T.push_back((2 * (int64_t)v + 1) * pow2(15 - ib));
    for (int x : bx) for (int y : by) out.push_back({x, y});
    solve(bx, gx, gy, yb, T, true, out);
    solve(by, gy, gx, xb, T, false, out);
}

// ---- the three forms as add_resident_16_regs computes them -----------------------------------------------------------------
struct Out { int wide, narrow; };
static int med3(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int16_t wrap16(int v) { return (int16_t)(uint16_t)(unsigned)v; }                 // what a 16-bit lane keeps
static int16_t half_of(unsigned rep) { return (int16_t)(uint16_t)(rep & 0xffffu); }     // one half of a replicated constant
static int16_t shl16(int16_t v, int n) { return wrap16((int)((unsigned)(uint16_t)v << n)); }
static int16_t add_sat16(int16_t a, int16_t b) { return (int16_t)med3((int)a + (int)b, -32768, 32767); }

// add_resident_16_pk: every lane 16 bits wide, constants from the replicated fields
static Out form_packed(int x, int y, int y_bytes, const AddResParams& p) {
    const int sx = half_of(p.shx2), sy = half_of(p.shy2), kk = half_of(p.k2);
    const int16_t lo = half_of(p.ilo2), hi = half_of(p.ihi2), hm1 = half_of(p.half2);
    const int16_t xs = shl16((int16_t)x, sx), ys = y_bytes == 2 ? (int16_t)y : shl16((int16_t)y, sy);
    const int16_t a = add_sat16(xs, ys);
    const int16_t s = a < lo ? lo : (a > hi ? hi : a);
    const int16_t bit = (int16_t)((s >> kk) & 1);
    const int16_t t = (int16_t)(wrap16(wrap16((int)s + (int)hm1) + (int)bit) >> kk);
    return {s, (int)(int8_t)(uint8_t)(med3(t, -128, 127) & 0xff)};
}

// add_resident_16_int<k > 0>: int32_t throughout; a left shift written as the multiplication it is, so that the sanitizer sees
// an overflow and a negative operand is defined
static Out form_int32(int x, int y, const AddResParams& p) {
    const int32_t S = med3(x * (int32_t(1) << p.shx) + y * (int32_t(1) << p.shy), p.ilo, p.ihi);
    const int32_t r = p.k > 0 ? (S + p.half_m1 + ((S >> p.k) & 1)) >> p.k : S * (int32_t(1) << -p.k);
    return {(int)(int16_t)(uint16_t)(S & 0xffff), (int)(int8_t)(uint8_t)(med3(r, -128, 127) & 0xff)};
}

// the fp32 chain (compiled without contraction, as the library is)
static float fmed3(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
static Out form_float(int x, int y, const AddResParams& p) {
    const float v = (float)x * p.sx + (float)y * p.sy;
    const float s = fmed3(v, p.lo, p.hi);
    const float q = fmed3(rintf(s * p.s_narrow), -128.0f, 127.0f);
    return {(int)(int16_t)(uint16_t)((unsigned)(int)(s * p.s_wide) & 0xffffu), (int)(int8_t)(uint8_t)((unsigned)(int)q & 0xffu)};
}

// the preconditions as the comments of fq_resident.h / fq_add_params.h state them, from (gx, gy, ib) alone
struct Q { int g, shx, shy, k; };
static Q quantities(int gx, int gy, int ib) { const int g = gx > gy ? (gx > 0 ? gx : 0) : (gy > 0 ? gy : 0); return {g, g - gx, g - gy, g - ib}; }
static bool pre_int32(const Q& q) { return q.g <= 8 && q.shx <= 12 && q.shy <= 12 && q.k >= -15 && q.k <= 24; }
static bool pre_packed(const Q& q, int xb, int yb) {
    return xb == 1 && q.g <= 8 && q.k >= 1 && q.k <= 8 && q.shx <= 8 && (yb == 1 ? q.shy <= 8 : q.shy == 0);
}

int main(int argc, char** argv) {
    Pairs pairs;
    if (argc == 7 && argv[1][0] == 'p') {
        boundary_pairs(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), pairs);
        for (auto& pr : pairs) printf("%d %d\n", pr.first, pr.second);
        return 0;
    }
    long sets = 0, evals = 0, selected[4] = {0, 0, 0, 0}, extra[4] = {0, 0, 0, 0};
    for (int gx = -16; gx <= 16; ++gx) for (int gy = -16; gy <= 16; ++gy) for (int ib = -16; ib <= 16; ++ib) {
        const Q q = quantities(gx, gy, ib);
        const bool wide = q.g <= 8;
        for (int xb = 1; xb <= 2; ++xb) for (int yb = 1; yb <= 2; ++yb) {
            boundary_pairs(xb, yb, gx, gy, ib, pairs);
            for (int relu = 0; relu <= 1; ++relu) {
                AddResParams p;
                if (make_add_params(gx, gy, q.g, wide, ib, relu, &p) != FQ_OK) { printf("make_add_params refuses %d %d %d\n", gx, gy, ib); return 1; }
                if (!wide && make_add_params(gx, gy, q.g, true, ib, relu, &p) != FQ_ERR_UNSUPPORTED) { printf("a wide sum at g = %d\n", q.g); return 1; }
                if (!wide) make_add_params(gx, gy, q.g, false, ib, relu, &p);
                if ((p.int_ok != 0) != pre_int32(q)) {       // (FQ_ADD_FLOAT / FQ_ADD_PACKED override the selection: run without them)
                    printf("int_ok %d against its stated condition at gx %d gy %d ib %d (is FQ_ADD_FLOAT set?)\n", p.int_ok, gx, gy, ib);
                    return 1;
                }
                const int sel = add_resident_form(p, xb, yb);
                const bool ok_sel = sel == kAddFormPacked ? pre_packed(q, xb, yb) : (sel == kAddFormFloat ? true : pre_int32(q) && (sel == kAddFormIntShift) == (q.k > 0));
                if (!ok_sel) { printf("FORM OUTSIDE ITS PROOF: form %d at gx %d gy %d ib %d x_bytes %d y_bytes %d\n", sel, gx, gy, ib, xb, yb); return 1; }
                ++sets; ++selected[sel];
                const bool run[4] = {true, pre_int32(q) && q.k <= 0, pre_int32(q) && q.k > 0, pre_packed(q, xb, yb)};
                for (int f = 0; f < 4; ++f) {
                    if (!run[f] && f != sel) continue;
                    if (f != sel) ++extra[f];
                    for (auto& pr : pairs) {
                        const int x = pr.first, y = pr.second;
                        const int64_t S = rule_sum(x, y, gx, gy, relu);
                        const int want_n = rule_narrow(S, ib);
                        int want_w = 0;
                        if (wide) {
                            if (S & (pow2(16 - q.g) - 1)) { printf("the rule's sum is off the wide grid\n"); return 1; }
                            want_w = (int)floor_div_pow2(S, 16 - q.g);
                        }
                        const Out o = f == kAddFormPacked ? form_packed(x, y, yb, p) : (f == kAddFormFloat ? form_float(x, y, p) : form_int32(x, y, p));
                        ++evals;
                        if (o.narrow != want_n || (wide && o.wide != want_w)) {
                            printf("MISMATCH form %d%s gx %d gy %d ib %d relu %d x_bytes %d y_bytes %d x %d y %d: wide %d want %d, narrow %d want %d\n", f,
                                   f == sel ? " (selected)" : "", gx, gy, ib, relu, xb, yb, x, y, o.wide, want_w, o.narrow, want_n);
                            return 1;
                        }
                    }
                }
            }
        }
    }
    printf("add_forms_check: OK %ld sets, %ld evaluations, selected fp32 %ld int32 %ld int32_shift %ld packed %ld, beside the selection %ld %ld %ld %ld\n", sets,
           evals, selected[0], selected[1], selected[2], selected[3], extra[0], extra[1], extra[2], extra[3]);
    return 0;
}
