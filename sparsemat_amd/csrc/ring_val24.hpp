// ring_val24.hpp -- K1r's 24-bit value code: f32 values that are all integer multiples k * 2^E of ONE power of two, with
// -2^23 <= k < 2^23, streamed as k (3 bytes) instead of the float (4 bytes).  Compiles for the host alone too
// (tests/cpp/ring_val24_on_host.cpp runs it under sanitizers).
//
// The unit is the 4-entry chunk of the element-anchored grid, as in ring_col12.hpp.  A chunk's four k take 12 bytes (24-bit two's
// complement, little-endian, contiguous); with the chunk's four low column bytes (ring_col12.hpp's `lo`: the bytes themselves, or
// the side-table index of an escaped chunk) that is one 16-byte record {w0, w1, w2, lo} -- what a lane loads for a chunk's values
// today, at the same byte offset.
//   value  = (float)k * 2^E           one conversion (exact: |k| <= 2^23) and one scaling by a power of two (exact: the bound on E
//                                     below keeps 2^E and every product a normal number)
// A value fits when that gives back its very bits.  +0.0f is k = 0; -0.0f, NaN, +-Inf and subnormals never fit; there are no
// per-value escapes: a matrix takes the code as a whole or not at all.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SMH_V24_HD __host__ __device__
#else
#define SMH_V24_HD
#endif

namespace smh {
namespace val24 {

// -100 <= E <= 100: 2^E and 2^-E are normal, and so is every |k| * 2^E with 1 <= |k| <= 2^23 (2^-100 .. 2^123)
constexpr int kMinExp = -100, kMaxExp = 100;
constexpr int32_t kMinK = -(1 << 23), kMaxK = (1 << 23) - 1;

SMH_V24_HD inline uint32_t float_bits(float v) {
    uint32_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}
SMH_V24_HD inline float bits_float(uint32_t b) {
    float v;
    memcpy(&v, &b, sizeof v);
    return v;
}

SMH_V24_HD inline bool exponent_ok(int E) { return E >= kMinExp && E <= kMaxExp; }
// 2^E as a float, built from its bits (E within the bound: a normal number)
SMH_V24_HD inline float scale_of(int E) { return bits_float((uint32_t)(E + 127) << 23); }

SMH_V24_HD inline float decode(int32_t k, float scale) { return (float)k * scale; }

// what the counting pass reduces, from a value's bits: is it one the code never holds (NaN, +-Inf, -0.0f, a subnormal) ...
SMH_V24_HD inline bool never_fits(uint32_t bits) {
    const uint32_t e = (bits >> 23) & 255u, m = bits & 0x7FFFFFu;
    return e == 255u || (e == 0u && m != 0u) || bits == 0x80000000u;
}
// ... and, of a normal value, the exponent of its lowest set mantissa bit (the implicit one included): the largest E it allows
SMH_V24_HD inline int lowest_bit_exponent(uint32_t bits) {
    const uint32_t sig = (bits & 0x7FFFFFu) | 0x800000u;
    return (int)((bits >> 23) & 255u) - 127 - 23 + __builtin_ctz(sig);
}

// v -> k with v == decode(k, 2^E) bit for bit; false: v does not fit (nothing is written)
SMH_V24_HD inline bool encode(float v, int E, int32_t *k_out) {
    if (!exponent_ok(E) || never_fits(float_bits(v))) return false;
    const float t = v * scale_of(-E);  // (overflow gives +-Inf, underflow a fraction or 0: neither passes below)
    if (!(t >= (float)kMinK && t <= (float)kMaxK)) return false;
    const int32_t k = (int32_t)t;
    if (float_bits(decode(k, scale_of(E))) != float_bits(v)) return false;
    *k_out = k;
    return true;
}
SMH_V24_HD inline bool fits(float v, int E) {
    int32_t k;
    return encode(v, E, &k);
}

// four k (each in [kMinK, kMaxK]) -> three dwords and back
SMH_V24_HD inline void pack(const int32_t (&k)[4], uint32_t (&w)[3]) {
    const uint32_t a = (uint32_t)k[0] & 0xFFFFFFu, b = (uint32_t)k[1] & 0xFFFFFFu, c = (uint32_t)k[2] & 0xFFFFFFu, d = (uint32_t)k[3] & 0xFFFFFFu;
    w[0] = a | b << 24;
    w[1] = b >> 8 | c << 16;
    w[2] = c >> 16 | d << 8;
}
SMH_V24_HD inline int32_t sext24(uint32_t x) { return (int32_t)(x << 8) >> 8; }
SMH_V24_HD inline void unpack(uint32_t w0, uint32_t w1, uint32_t w2, int32_t (&k)[4]) {
    k[0] = sext24(w0);
    k[1] = sext24(w0 >> 24 | w1 << 8);
    k[2] = sext24(w1 >> 16 | w2 << 16);
    k[3] = (int32_t)w2 >> 8;
}

// a record's three value dwords -> the chunk's four values
SMH_V24_HD inline void decode_chunk(uint32_t w0, uint32_t w1, uint32_t w2, float scale, float (&v)[4]) {
    int32_t k[4];
    unpack(w0, w1, w2, k);
    for (int q = 0; q < 4; ++q) v[q] = decode(k[q], scale);
}

}  // namespace val24
}  // namespace smh
