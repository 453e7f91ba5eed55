// ring_col12.hpp -- K1r's compact column form: 12 bits per entry instead of the 16 of `col16`, for f32 matrices on the
// 16384-slot single-window ring.  Compiles for the host alone too (tests/cpp/ring_col12_on_host.cpp runs it under sanitizers).
//
// The unit is the 4-entry chunk of the element-anchored grid (the grid of the kernel's 16-byte value loads).  With
// slot_q = column_q mod 16384 (q = 0..3), a slot is a 6-bit stratum (slot >> 8) over a low byte:
//   lo8[4c + q] = slot_q & 255                      one byte per entry, a chunk's four read as one dword
//   hdr[c]      = h0 << 10 | t                      one u16 per chunk: h0 = stratum of slot_0, t = rank of (d1, d2, d3),
//                                                   d_q = (stratum_q - h0) mod 64, among the non-decreasing triples with d3 <= 16
// Sorted rows inside a window of at most 16384 columns give such triples (the mod-64 difference also covers the window's wrap
// around the ring).  There are C(19, 3) = 969 of them, so t takes 10 bits, and a table of 969 u16 turns t back into the triple.
// A chunk the code cannot hold (wider span, columns not ascending -- a chunk that straddles two rows usually is one) gets
// t = 1023 and, in place of its four low bytes, an index into a side table of 4 x u16 true slots.
// Every chunk decodes on its own, from byte-aligned loads, to the very slots `column mod 16384` gives.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SMH_C12_HD __host__ __device__
#else
#define SMH_C12_HD
#endif

namespace smh {
namespace col12 {

constexpr uint32_t kSlots = 16384;      // the ring this form is defined for
constexpr uint32_t kMaxGap = 16;        // largest stratum distance from slot_0 a header can hold
constexpr uint32_t kTriples = 969;      // C(19, 3)
constexpr uint32_t kEscape = 1023;      // t of a chunk whose slots come from the side table
constexpr uint32_t kTableEntries = 1024;  // the table as stored (2 KiB): entries past kTriples are zero

// rank of a non-decreasing triple: the combinatorial number of the strictly increasing (d1, d2 + 1, d3 + 2)
SMH_C12_HD constexpr uint32_t triple_rank(uint32_t d1, uint32_t d2, uint32_t d3) {
    return d1 + (d2 + 1) * d2 / 2 + (d3 + 2) * (d3 + 1) * d3 / 6;
}
// a table entry: three 5-bit fields
SMH_C12_HD constexpr uint16_t pack_triple(uint32_t d1, uint32_t d2, uint32_t d3) { return (uint16_t)(d1 | d2 << 5 | d3 << 10); }

struct Table {
    uint16_t e[kTableEntries];
};
constexpr Table make_table() {
    Table t{};
    for (uint32_t d3 = 0; d3 <= kMaxGap; ++d3)
        for (uint32_t d2 = 0; d2 <= d3; ++d2)
            for (uint32_t d1 = 0; d1 <= d2; ++d1) t.e[triple_rank(d1, d2, d3)] = pack_triple(d1, d2, d3);
    return t;
}

// slots (each < kSlots) -> header and low bytes; false: the code cannot hold this chunk (nothing is written)
SMH_C12_HD inline bool encode_chunk(const uint32_t (&slot)[4], uint16_t *hdr, uint32_t *lo) {
    const uint32_t h0 = slot[0] >> 8;
    const uint32_t d1 = ((slot[1] >> 8) - h0) & 63u, d2 = ((slot[2] >> 8) - h0) & 63u, d3 = ((slot[3] >> 8) - h0) & 63u;
    if (!(d1 <= d2 && d2 <= d3 && d3 <= kMaxGap)) return false;
    *hdr = (uint16_t)(h0 << 10 | triple_rank(d1, d2, d3));
    *lo = (slot[0] & 255u) | (slot[1] & 255u) << 8 | (slot[2] & 255u) << 16 | (slot[3] & 255u) << 24;
    return true;
}

SMH_C12_HD inline bool is_escape(uint32_t hdr) { return (hdr & 1023u) == kEscape; }

// header and low bytes -> slots, `table` = Table::e.  Of an escaped chunk (and of any bit pattern) this gives slots
// below kSlots too -- meaningless ones: the caller replaces them from the side table.
SMH_C12_HD inline void decode_chunk(uint32_t hdr, uint32_t lo, const uint16_t *table, uint32_t (&slot)[4]) {
    const uint32_t h0 = (hdr >> 10) & 63u;
    const uint32_t e = table[hdr & 1023u];
    slot[0] = h0 << 8 | (lo & 255u);
    slot[1] = ((h0 + (e & 31u)) & 63u) << 8 | ((lo >> 8) & 255u);
    slot[2] = ((h0 + ((e >> 5) & 31u)) & 63u) << 8 | ((lo >> 16) & 255u);
    slot[3] = ((h0 + ((e >> 10) & 31u)) & 63u) << 8 | (lo >> 24);
}

// a side-table entry: the four true slots as two packed pairs
SMH_C12_HD inline void pack_escape(const uint32_t (&slot)[4], uint32_t (&pair)[2]) {
    pair[0] = slot[0] | slot[1] << 16;
    pair[1] = slot[2] | slot[3] << 16;
}
SMH_C12_HD inline void unpack_escape(uint32_t p0, uint32_t p1, uint32_t (&slot)[4]) {
    slot[0] = p0 & (kSlots - 1u);
    slot[1] = (p0 >> 16) & (kSlots - 1u);
    slot[2] = p1 & (kSlots - 1u);
    slot[3] = (p1 >> 16) & (kSlots - 1u);
}

}  // namespace col12
}  // namespace smh
