// Host check of csrc/lrg_text_fmt.h, the arithmetic both passes of lrg_text.hip share: every line it builds is compared with snprintf's
// "%f" / "%d" (correctly rounded, ties to even, as Python's '%' operator).  Plain C++, no GPU:
//   c++ -std=c++17 -O2 [-fsanitize=address,undefined] tools/text_fmt_check.cpp -o text_fmt_check && ./text_fmt_check [values]
// Prints "ok <rows> rows" and exits 0, or the first mismatches and exits 1.  tests/test_text_host.py builds and runs it.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../learn_region_grow_amd/csrc/lrg_text_fmt.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                                      // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static long rows = 0, bad = 0;

static void check_row(const float x[3], const int32_t rgb[3], int format) {
    uint8_t got[LRG_TEXT_MAX_LINE + 32];
    char want[256];
    const uint32_t bits[3] = {to_bits(x[0]), to_bits(x[1]), to_bits(x[2])};
    LrgTextRow r;
    lrg_text_row(bits, rgb, format, &r);
    ++rows;
    bool refuse = false;
    for (int k = 0; k < 3; ++k) refuse = refuse || !(fabs((double)x[k]) < 1099511627776.0);
    if (format == LRG_TEXT_PCD)
        for (int k = 0; k < 3; ++k) refuse = refuse || rgb[k] < 0 || rgb[k] > 255;
    if (refuse) {
        if (r.len != 0 && ++bad < 10) printf("not refused: %a %a %a\n", x[0], x[1], x[2]);
        return;
    }
    int n;
    if (format == LRG_TEXT_PCD)
        n = snprintf(want, sizeof want, "%f %f %f %d\n", (double)x[0], (double)x[1], (double)x[2], (rgb[0] << 16) | (rgb[1] << 8) | rgb[2]);
    else
        n = snprintf(want, sizeof want, "%f %f %f %d %d %d\n", (double)x[0], (double)x[1], (double)x[2], rgb[0], rgb[1], rgb[2]);
    memset(got, '#', sizeof got);
    if (r.len > 0 && r.len <= LRG_TEXT_MAX_LINE) lrg_text_put_row(got, r);
    if (r.len != n || n > LRG_TEXT_MAX_LINE || memcmp(got, want, (size_t)n) != 0 || got[n] != '#') {
        if (++bad < 10) printf("mismatch (len %d, want %d): %.*s", r.len, n, n, want);
    }
}

static void check_value(float v) {
    static const int32_t cols[][3] = {{0, 255, 7}, {100, 100, 100}, {INT32_MIN, -1, INT32_MAX}, {9, 10, 99}, {1000, 65536, 123456789}};
    static int turn = 0;
    const float a[3] = {v, -v, v}, b[3] = {0.0f, v, 1.5f};
    check_row(a, cols[turn % 5], LRG_TEXT_PLY);
    check_row(b, cols[(turn + 1) % 5], turn % 2 ? LRG_TEXT_PCD : LRG_TEXT_PLY);
    ++turn;
}

int main(int argc, char **argv) {
    const long count = argc > 1 ? atol(argv[1]) : 200000;
    const float picked[] = {0.0f, -0.0f, 1e-9f, -1e-9f, 5e-7f, nextafterf(5e-7f, 0.0f), nextafterf(5e-7f, 1.0f), 4.9999997e-7f, 0.9999995f, 9.9999995f,
                            999999.97f, 1e-45f, 123456.789f, 549755813888.0f, 0.0078125f, 0.0234375f, 1099511562240.0f, -1099511562240.0f,
                            1099511627776.0f, INFINITY, -INFINITY, NAN, 1.17549435e-38f, 1e-40f, 0.5f, 1.0f, 16777216.0f, 3.4e38f};
    for (float v : picked) check_value(v);
    for (int k = -(1 << 20); k <= (1 << 20); ++k) check_value((float)k / 128.0f);            // every multiple of 1/128 in +-2^13: the odd ones are exact ties
    for (int k = 1; k < 4096; k += 2)
        for (int d = -1; d <= 1; d += 2) check_value(nextafterf((float)k / 128.0f, d * 1e9f));
    for (long k = 0; k < count; ++k) {                                                        // random bit patterns below 2^40, subnormals included
        uint32_t b = rnd();
        b = (b & 0x807fffffu) | ((rnd() % 167u) << 23);
        check_value(from_bits(b));
    }
    for (long k = 0; k < count; ++k) {                                                        // room-sized coordinates
        const float u = (float)(rnd() >> 8) / 16777216.0f;
        check_value((u - 0.5f) * 40.0f);
    }
    const float ext[3] = {-1099511562240.0f, -1099511562240.0f, -1099511562240.0f};           // -(2^40 - 2^16): the longest line there is
    const int32_t mn[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    LrgTextRow r;
    const uint32_t eb[3] = {to_bits(ext[0]), to_bits(ext[1]), to_bits(ext[2])};
    lrg_text_row(eb, mn, LRG_TEXT_PLY, &r);
    if (r.len != LRG_TEXT_MAX_LINE) { printf("longest line: %d bytes, LRG_TEXT_MAX_LINE %d\n", r.len, LRG_TEXT_MAX_LINE); ++bad; }
    check_row(ext, mn, LRG_TEXT_PLY);
    if (bad) { printf("%ld of %ld rows differ\n", bad, rows); return 1; }
    printf("ok %ld rows\n", rows);
    return 0;
}
