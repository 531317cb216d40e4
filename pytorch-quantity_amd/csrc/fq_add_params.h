// fq_add_params.h -- the host side of the resident NewAdd (add_resident_16_regs in fq_resident.h): its parameter record, the
// function that fills it and thereby SELECTS one of the three arithmetic forms, and the form's number for tests.  No HIP
// dependency, so the same selection compiles as host code: scripts/add_forms_check.cpp runs it over every (gx, gy, ib, relu,
// operand types) and holds each form, written out in plain C++, against the rule in 64-bit integers.
#pragma once
#include <cmath>
#include <cstdlib>
#include "../../include/fq.h"

namespace fq {

struct AddResParams {
    float sx, sy;          // 2^-gx, 2^-gy: integer -> value
    float lo, hi;          // NewAdd's Sp range; lo = 0 when the following ReLU is fused
    float s_wide;          // 2^g_out   (exact value -> int16)
    float s_narrow;        // 2^ib      (next layers' Quantity)
    // the same function in integer arithmetic on the grid g = max(0, gx, gy) (int_ok: the host proved the ranges)
    int int_ok;
    int shx, shy;          // g - gx, g - gy: operand -> grid g
    int ilo, ihi;          // Sp range on grid g
    int k, half_m1;        // narrow = S * 2^(ib - g): k = g - ib; k > 0: round-half-even right shift with 2^(k-1) - 1
    // the integer form on PAIRS of int16 (v_pk_*_i16: two elements per instruction) where every intermediate fits 16 bits:
    // pk_ok8 / pk_ok16 for an int8 / int16 operand y; the constants below are the ones above, replicated in both halves
    int pk_ok8, pk_ok16;
    unsigned shx2, shy2, k2, ilo2, ihi2, half2;
};

// host: parameters of one resident add; FQ_OK or an error code (ranges, exact-sum grid)
inline int make_add_params(int gx, int gy, int g_wide, bool want_wide, int ib, int relu, AddResParams* p) {
    if (gx < -16 || gx > 16 || gy < -16 || gy > 16 || ib < -16 || ib > 16) return FQ_ERR_INVALID_ARG;
    if (want_wide) {
        // the exact sum must fit: grid max(0, gx, gy), |s| <= 128  =>  |S| <= 2^(7 + g) <= 2^15
        const int g_need = gx > gy ? (gx > 0 ? gx : 0) : (gy > 0 ? gy : 0);
        if (g_wide != g_need || g_wide > 8) return FQ_ERR_UNSUPPORTED;
    }
    p->sx = ldexpf(1.0f, -gx); p->sy = ldexpf(1.0f, -gy);
    p->lo = relu ? 0.0f : -128.0f; p->hi = 127.0f;
    p->s_wide = ldexpf(1.0f, want_wide ? g_wide : 0); p->s_narrow = ldexpf(1.0f, ib);
    // integer form: operands |x|, |y| <= 2^15 shifted by at most 12, the clamped sum |S| <= 2^(7+g) <= 2^15 shifted left by
    // at most 15 -- nothing leaves int32.  FQ_ADD_FLOAT=1 keeps the fp32 chain (A/B timing).
    static const bool force_float = [] { const char* e = getenv("FQ_ADD_FLOAT"); return e && e[0] && e[0] != '0'; }();
    const int g = gx > gy ? (gx > 0 ? gx : 0) : (gy > 0 ? gy : 0);
    p->shx = g - gx; p->shy = g - gy;
    p->k = g - ib;
    p->int_ok = !force_float && g <= 8 && p->shx <= 12 && p->shy <= 12 && p->k >= -15 && p->k <= 24;
    p->ilo = relu ? 0 : -(128 << g); p->ihi = 127 << g;
    if (!p->int_ok) { p->shx = p->shy = 0; p->k = 0; }
    p->half_m1 = p->k > 0 ? (1 << (p->k - 1)) - 1 : 0;    // (behind the line above: k - 1 <= 23, where k itself reaches 32)
    // packed int16 form: every intermediate inside 16 bits (see add_resident_16_pk).  FQ_ADD_PACKED=0 keeps the 32-bit form.
    static const bool no_pk = [] { const char* e = getenv("FQ_ADD_PACKED"); return e && e[0] == '0'; }();
    const bool pk = p->int_ok && !no_pk && p->k >= 1 && p->k <= 8 && p->shx >= 0 && p->shx <= 8;
    p->pk_ok8 = pk && p->shy >= 0 && p->shy <= 8;
    p->pk_ok16 = pk && p->shy == 0;
    auto rep = [](int v) { return ((unsigned)v & 0xffffu) * 0x10001u; };
    p->shx2 = rep(p->shx); p->shy2 = rep(p->shy); p->k2 = rep(p->k); p->ilo2 = rep(p->ilo); p->ihi2 = rep(p->ihi);
    p->half2 = rep(p->half_m1);
    return FQ_OK;
}

// Which form add_resident_16_regs runs for these parameters and operand types, branch for branch (a diagnostic for tests,
// fq_add_resident_form): the packed form needs an int8 x and pk_ok8 / pk_ok16 by y's type, then the 32-bit form by the sign of k.
constexpr int kAddFormFloat = 0, kAddFormInt = 1, kAddFormIntShift = 2, kAddFormPacked = 3;

inline int add_resident_form(const AddResParams& p, int x_bytes, int y_bytes) {
    if (x_bytes == 1 && (y_bytes == 2 ? p.pk_ok16 : p.pk_ok8)) return kAddFormPacked;
    if (p.int_ok) return p.k > 0 ? kAddFormIntShift : kAddFormInt;
    return kAddFormFloat;
}

}  // namespace fq
