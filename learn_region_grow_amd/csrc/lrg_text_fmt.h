// '%f' of a float32 and '%d' of an int32 as Python's '%' operator prints them, in integer arithmetic alone: shared by the
// two passes of lrg_text.hip and, compiled for the host, by tools/text_fmt_check.cpp, which reads it against printf.
//
// A float32 is m 2^e with m < 2^24, so x 10^6 = (m 15625) 2^(e + 6) with m 15625 < 2^38: a 64-bit integer shifted left (exact) or right
// (one round-half-even on the bits shifted out), which is the correctly rounded six-decimal value '%f' prints after widening to double.
#pragma once
#include <stdint.h>
#include "../../include/lrg_hip.h"

#ifdef __HIPCC__
#define LRG_TEXT_FN __host__ __device__ __forceinline__
#else
#define LRG_TEXT_FN static inline
#endif

struct LrgTextNum { uint64_t q; int sign, nd; };      // |x| 10^6 rounded; the sign BIT; decimal digits of q, at least 7 ("0.000000")
struct LrgTextRow { LrgTextNum c[3]; int32_t col[3]; int ncol, len; };      // len == 0: the row is refused

LRG_TEXT_FN int lrg_text_digits_u32(uint32_t v) {
    return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 :
           v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}

// false: not finite, or |x| >= 2^40 (q would pass 2^60)
LRG_TEXT_FN bool lrg_text_f32(uint32_t bits, LrgTextNum *o) {
    const int ex = (int)((bits >> 23) & 0xffu);
    const uint32_t man = bits & 0x7fffffu;
    if (ex >= 127 + 40) return false;
    const uint64_t N = (uint64_t)(ex ? (man | 0x800000u) : man) * 15625u;
    const int s = (ex ? ex - 150 : -149) + 6;
    uint64_t q;
    if (s >= 0) q = N << s;                                  // s <= 22 and N < 2^38
    else if (-s >= 64) q = 0;                                // N < 2^38 is below half of 2^63
    else {
        const int k = -s;
        const uint64_t rem = N & ((1ull << k) - 1), half = 1ull << (k - 1);
        q = N >> k;
        if (rem > half || (rem == half && (q & 1))) ++q;
    }
    o->q = q;
    o->sign = (int)(bits >> 31);
    const uint32_t hi = (uint32_t)(q / 1000000000u);         // q < 2^60 < 1.16e18: one split, two 32-bit halves
    const int nd = hi ? 9 + lrg_text_digits_u32(hi) : lrg_text_digits_u32((uint32_t)q);
    o->nd = nd < 7 ? 7 : nd;
    return true;
}

LRG_TEXT_FN int lrg_text_len_f(const LrgTextNum &v) { return v.sign + v.nd + 1; }
LRG_TEXT_FN int lrg_text_len_d(int32_t v) { return (v < 0) + lrg_text_digits_u32(v < 0 ? 0u - (uint32_t)v : (uint32_t)v); }

// the field at p; returns the byte behind it
LRG_TEXT_FN uint8_t *lrg_text_put_f(uint8_t *p, const LrgTextNum &v) {
    if (v.sign) *p++ = '-';
    uint8_t *const end = p + v.nd + 1;
    uint8_t *w = end;
    uint32_t hi = (uint32_t)(v.q / 1000000000u), lo = (uint32_t)(v.q % 1000000000u);
    const int nlo = hi ? 9 : v.nd;
    int k = 0;
    for (; k < nlo; ++k) {
        if (k == 6) *--w = '.';
        *--w = (uint8_t)('0' + lo % 10u);
        lo /= 10u;
    }
    for (; k < v.nd; ++k) {                                  // (k >= 9 here: the point is behind us)
        *--w = (uint8_t)('0' + hi % 10u);
        hi /= 10u;
    }
    return end;
}

LRG_TEXT_FN uint8_t *lrg_text_put_d(uint8_t *p, int32_t v) {
    uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    if (v < 0) *p++ = '-';
    const int nd = lrg_text_digits_u32(a);
    uint8_t *const end = p + nd;
    uint8_t *w = end;
    for (int k = 0; k < nd; ++k) {
        *--w = (uint8_t)('0' + a % 10u);
        a /= 10u;
    }
    return end;
}

// What one row prints: its three coordinates, its colour fields and the length of its line (0 = refused)
LRG_TEXT_FN void lrg_text_row(const uint32_t xyz_bits[3], const int32_t rgb[3], int format, LrgTextRow *r) {
    bool ok = true;
    int len = 0;
    for (int k = 0; k < 3; ++k) {
        ok = lrg_text_f32(xyz_bits[k], &r->c[k]) && ok;
        if (ok) len += lrg_text_len_f(r->c[k]) + 1;
    }
    if (format == LRG_TEXT_PCD) {
        ok = ok && (uint32_t)rgb[0] < 256u && (uint32_t)rgb[1] < 256u && (uint32_t)rgb[2] < 256u;
        r->ncol = 1;
        r->col[0] = (int32_t)(((uint32_t)rgb[0] << 16) | ((uint32_t)rgb[1] << 8) | (uint32_t)rgb[2]);
        r->col[1] = r->col[2] = 0;
    } else {
        r->ncol = 3;
        for (int k = 0; k < 3; ++k) r->col[k] = rgb[k];
    }
    for (int k = 0; k < r->ncol; ++k) len += lrg_text_len_d(r->col[k]) + 1;
    r->len = ok ? len : 0;
}

LRG_TEXT_FN void lrg_text_put_row(uint8_t *p, const LrgTextRow &r) {
    for (int k = 0; k < 3; ++k) {
        p = lrg_text_put_f(p, r.c[k]);
        *p++ = ' ';
    }
    for (int k = 0; k < r.ncol; ++k) {
        p = lrg_text_put_d(p, r.col[k]);
        *p++ = k + 1 < r.ncol ? ' ' : '\n';
    }
}
