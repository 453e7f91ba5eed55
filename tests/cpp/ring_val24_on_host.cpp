// ring_val24_on_host.cpp -- K1r's 24-bit value code (sparsemat_amd/csrc/ring_val24.hpp: the functions the encoder kernels and the
// ring kernel call) on the host, built with -fsanitize=address,undefined by tests/test_ring_val24_host.py:
//   1. all 2^24 integers k round-trip at E = -23 -- against the synthetic generator's own formula (float)u * 2^-23 - 1, u = k + 2^23,
//      bit for bit --, at E = 0 and at E = -21, through encode / pack / unpack / decode in chunks of four, as the kernels do;
//   2. random quadruples pack and unpack to themselves, with the extremes -2^23 and 2^23 - 1 in every position;
//   3. what never fits is refused: -0.0f, NaN, +-Inf, subnormals, 0.1f, 2^23 * 2^E (one past the range), a value whose lowest set
//      bit lies below E, an exponent outside the stated bound; and the two functions of the counting pass agree with fits().
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>

#include "ring_val24.hpp"

using namespace smh::val24;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++failures <= 20) printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
        }                                                                  \
    } while (0)

// every k in chunks of four: value -> encode -> pack -> unpack -> decode_chunk gives the value's bits
static void all_integers(int E, bool generator_formula) {
    const float scale = scale_of(E);
    CHECK(scale == std::ldexp(1.0f, E));
    for (int64_t base = kMinK; base <= kMaxK; base += 4) {
        float v[4];
        int32_t k[4], back[4];
        for (int q = 0; q < 4; ++q) {
            const int32_t want = (int32_t)(base + q);
            // E = -23: what hash_to_unit<float> draws from 24 bits u
            v[q] = generator_formula ? (float)(uint32_t)(want + (1 << 23)) * 0x1p-23f - 1.0f : std::ldexp((float)want, E);
            k[q] = 0x7FFFFFFF;
            CHECK(fits(v[q], E));
            CHECK(encode(v[q], E, &k[q]) && k[q] == want);
            CHECK(float_bits(decode(k[q], scale)) == float_bits(v[q]));
            if (v[q] != 0.0f) CHECK(lowest_bit_exponent(float_bits(v[q])) >= E);
            CHECK(!never_fits(float_bits(v[q])));
        }
        uint32_t w[3];
        pack(k, w);
        unpack(w[0], w[1], w[2], back);
        float got[4];
        decode_chunk(w[0], w[1], w[2], scale, got);
        for (int q = 0; q < 4; ++q) {
            CHECK(back[q] == k[q]);
            CHECK(float_bits(got[q]) == float_bits(v[q]));
        }
    }
}

static void quadruples() {
    std::mt19937 rng(24);
    std::uniform_int_distribution<int32_t> any(kMinK, kMaxK);
    const int32_t extremes[] = {kMinK, kMaxK, 0, -1, 1};
    for (int it = 0; it < 200000; ++it) {
        int32_t k[4] = {any(rng), any(rng), any(rng), any(rng)}, back[4];
        if (it < 4 * 5 * 5) {  // an extreme in position it % 4, another in the position after it
            k[it % 4] = extremes[(it / 4) % 5];
            k[(it + 1) % 4] = extremes[(it / 20) % 5];
        }
        uint32_t w[3];
        pack(k, w);
        unpack(w[0], w[1], w[2], back);
        for (int q = 0; q < 4; ++q) CHECK(back[q] == k[q]);
        // the bytes are the four 24-bit integers, little-endian, one after the other
        for (int q = 0; q < 4; ++q)
            for (int b = 0; b < 3; ++b) {
                const int byte = 3 * q + b;
                CHECK(((w[byte / 4] >> (8 * (byte % 4))) & 255u) == (((uint32_t)k[q] >> (8 * b)) & 255u));
            }
    }
    for (int pos = 0; pos < 4; ++pos)
        for (int32_t e : {kMinK, kMaxK}) {
            int32_t k[4] = {0, 0, 0, 0}, back[4];
            k[pos] = e;
            uint32_t w[3];
            pack(k, w);
            unpack(w[0], w[1], w[2], back);
            for (int q = 0; q < 4; ++q) CHECK(back[q] == k[q]);
        }
}

static void refusals() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float sub = std::numeric_limits<float>::denorm_min(), sub2 = bits_float(0x007FFFFFu);
    for (int E : {-23, 0, -21, kMinExp, kMaxExp}) {
        int32_t k = 77;
        for (float v : {-0.0f, nan, -nan, inf, -inf, sub, -sub, sub2}) {
            CHECK(!fits(v, E));
            CHECK(!encode(v, E, &k) && k == 77);
            CHECK(never_fits(float_bits(v)));
        }
        CHECK(fits(0.0f, E) && encode(0.0f, E, &k) && k == 0);
        CHECK(!fits(std::ldexp(8388608.0f, E), E));    // 2^23 * 2^E: one past the range
        CHECK(fits(std::ldexp(8388607.0f, E), E));
        CHECK(fits(std::ldexp(-8388608.0f, E), E));
        CHECK(!fits(std::ldexp(-8388609.0f, E), E));   // (a 24-bit significand: exact as a float)
        CHECK(!fits(std::ldexp(1.0f, E - 1), E));      // the lowest set bit lies below E
        CHECK(!fits(std::ldexp(3.0f, E - 1), E));
        CHECK(!fits(std::ldexp(16777215.0f, E - 1), E));
        CHECK(fits(std::ldexp(1.0f, E), E) && fits(std::ldexp(1.0f, E + 22), E) && !fits(std::ldexp(1.0f, E + 23), E));
    }
    CHECK(!fits(0.1f, -23) && !fits(0.1f, -27) && !fits(0.1f, -100) && !never_fits(float_bits(0.1f)));
    CHECK(lowest_bit_exponent(float_bits(0.1f)) == -27);  // 0.1f = 13421773 * 2^-27: 24 significant bits, and k would be 2^23 and more
    // an exponent outside the bound refuses everything, zero and representable values included
    for (int E : {kMinExp - 1, kMaxExp + 1, -127, 128, 1000, -1000}) {
        CHECK(!exponent_ok(E));
        CHECK(!fits(0.0f, E) && !fits(1.0f, E) && !fits(std::ldexp(1.0f, E > 0 ? 127 : -126), E));
    }
    CHECK(exponent_ok(kMinExp) && exponent_ok(kMaxExp));
    // values far from 2^E on either side neither overflow into a fit nor trap
    CHECK(!fits(std::numeric_limits<float>::max(), kMinExp) && !fits(std::numeric_limits<float>::min(), kMaxExp));
    // the counting pass's exponent: the largest E a value is a multiple of 2^E for
    std::mt19937 rng(7);
    for (int it = 0; it < 200000; ++it) {
        const uint32_t bits = (uint32_t)rng();
        if (never_fits(bits) || (bits & 0x7FFFFFFFu) == 0u) continue;
        const float v = bits_float(bits);
        const int e = lowest_bit_exponent(bits);
        CHECK(std::ldexp(std::nearbyint(std::ldexp(v, -e)), e) == v);  // a multiple of 2^e ...
        const float half = std::ldexp(v, -e - 1);                       // ... and of no higher power
        if (std::isfinite(half) && std::fabs(half) < 0x1p60f && std::fabs(half) >= 0x1p-60f) CHECK(std::nearbyint(half) != half);
        // v / 2^e is an odd integer of at most 24 bits: it fits when that integer is in the 24-bit two's complement range
        const float t = std::ldexp(v, -e);
        if (exponent_ok(e)) CHECK(fits(v, e) == (t >= -8388608.0f && t <= 8388607.0f));
    }
}

int main() {
    all_integers(-23, true);
    all_integers(-23, false);
    all_integers(0, false);
    all_integers(-21, false);
    quadruples();
    refusals();
    printf("ring_val24_on_host: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
