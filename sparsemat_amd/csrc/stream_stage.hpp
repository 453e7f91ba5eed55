// stream_stage.hpp -- what the K1s family (spmv_stream.hip, spmv_stream_xd.hip) and the builders of its code arrays must agree on,
// written once: the layout of a tile's LDS stage of x, the bits of a 16-bit stage-offset code, the XCD tile map and the rounded
// multiply / add.  Compiles for the host alone too (tests/cpp/stream_stage_on_host.cpp runs the layout and the codes under sanitizers).
//
// THE STAGE.  The inspector (k_stream_windows) describes the columns a 256-row tile references as up to 4 sorted, disjoint intervals
// [a_q, e_q) -- 8 table words; e_q <= a_q: unused, the used ones are a prefix.  The stage holds the used intervals back to back, each
// from its 4-aligned start al_q = a_q & ~3 in whole 16-byte chunks of 4 entries: interval q takes n_q = ceil((e_q - al_q) / 4) chunks
// from stage chunk p_q = n_0 + .. + n_(q-1) on.  Five places read this layout: the fills of k_spmv_stream_xd, k_spmv_stream_xdp and
// k_spmv_stream's XS body (stage chunk -> chunk of x), k_stream_stage_codes (column -> stage entry, times the element size: the code)
// and k_stream_xs_stats (chunks and end: the host's promise to the kernels that the stage fits and that the chunk loads stay inside x).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SMH_STAGE_HD __host__ __device__ __forceinline__
#else
#define SMH_STAGE_HD inline
#endif

namespace smh {
namespace stage {

// (scalar members, no arrays: with arrays the compiler kept the select chains of entry() as indexed loads from a per-thread copy)
struct Layout {
    uint32_t a0, a1, a2, a3;  // the intervals' first columns, as the table has them
    uint32_t p1, p2, p3, p4;  // first stage chunk of intervals 1..3 (interval 0 starts the stage) and p4 = chunks of the whole stage;
                              // p_(q+1) == p_q: interval q is unused

    SMH_STAGE_HD uint32_t chunks() const { return p4; }
    // the largest x index + 1 the chunk loads touch (0: no chunk)
    SMH_STAGE_HD uint32_t end() const {
        const uint32_t e0 = end_of(a0, 0u, p1), e1 = end_of(a1, p1, p2), e2 = end_of(a2, p2, p3), e3 = end_of(a3, p3, p4);
        const uint32_t e01 = e0 > e1 ? e0 : e1, e23 = e2 > e3 ? e2 : e3;
        return e01 > e23 ? e01 : e23;
    }
    // stage chunk j (< chunks()) -> chunk of x: j + d_q with the tile-uniform d_q = al_q / 4 - p_q (mod 2^32), q = the interval j falls
    // into.  Three selects: the kernels that call this per chunk are bound by vector-ALU issue.
    SMH_STAGE_HD uint32_t x_chunk(uint32_t j) const {
        uint32_t d = a0 >> 2;
        d = j >= p1 ? (a1 >> 2) - p1 : d;
        d = j >= p2 ? (a2 >> 2) - p2 : d;
        d = j >= p3 ? (a3 >> 2) - p3 : d;
        return j + d;
    }
    // column c of the tile -> index of x[c] in the stage (the used intervals are a prefix of the table, sorted, disjoint, and contain c)
    SMH_STAGE_HD uint32_t entry(uint32_t c) const {
        const uint32_t q = (uint32_t)(p2 != p1 && c >= a1) + (uint32_t)(p3 != p2 && c >= a2) + (uint32_t)(p4 != p3 && c >= a3);
        const uint32_t al = (q == 3u ? a3 : q == 2u ? a2 : q == 1u ? a1 : a0) & ~3u;
        const uint32_t pq = q == 3u ? p3 : q == 2u ? p2 : q == 1u ? p1 : 0u;
        return 4u * pq + (c - al);
    }
    // where the first columns of the four intervals sit: entry(a_q) with q known (the XS body adds a column code's 14-bit offset)
    SMH_STAGE_HD uint32_t first_entry0() const { return a0 & 3u; }
    SMH_STAGE_HD uint32_t first_entry1() const { return 4u * p1 + (a1 & 3u); }
    SMH_STAGE_HD uint32_t first_entry2() const { return 4u * p2 + (a2 & 3u); }
    SMH_STAGE_HD uint32_t first_entry3() const { return 4u * p3 + (a3 & 3u); }

    // chunks of [a, e) from its aligned start; one past the last x index of an interval that takes stage chunks [pa, pb)
    SMH_STAGE_HD static uint32_t chunks_of(uint32_t a, uint32_t e) { return e > a ? (e - (a & ~3u) + 3u) >> 2 : 0u; }
    SMH_STAGE_HD static uint32_t end_of(uint32_t a, uint32_t pa, uint32_t pb) { return pb != pa ? (a & ~3u) + 4u * (pb - pa) : 0u; }
};

// w: the tile's 8 table words
SMH_STAGE_HD Layout layout(const uint32_t *w) {
    Layout l;
    l.a0 = w[0]; l.a1 = w[2]; l.a2 = w[4]; l.a3 = w[6];
    l.p1 = Layout::chunks_of(l.a0, w[1]);
    l.p2 = l.p1 + Layout::chunks_of(l.a1, w[3]);
    l.p3 = l.p2 + Layout::chunks_of(l.a2, w[5]);
    l.p4 = l.p3 + Layout::chunks_of(l.a3, w[7]);
    return l;
}

// THE CODE.  K1s XD's 16-bit code is the BYTE offset of x[column] in the stage: a multiple of the element size below the stage's
// xs * 1024 entries.  That leaves bits to spare -- the low log2(element size) ones and those from code_high_shift up -- and K1s XD-V
// keeps an entry's value-dictionary index there: in the low and the high ones (`low` = code_low_bits), or, when the index fits them,
// in the high ones alone (`low` = 0: one shift decodes it).
SMH_STAGE_HD constexpr uint32_t code_low_bits(uint32_t elem_bytes) { return elem_bytes == 8 ? 3u : 2u; }
SMH_STAGE_HD constexpr uint32_t code_index_bits(int xs) { return xs == 4 ? 12u : 11u; }  // bits of an entry index inside the stage
SMH_STAGE_HD constexpr uint32_t code_high_shift(uint32_t elem_bytes, int xs) { return code_low_bits(elem_bytes) + code_index_bits(xs); }
SMH_STAGE_HD constexpr uint32_t code_ofs_mask(uint32_t elem_bytes, int xs) {
    return ((1u << code_high_shift(elem_bytes, xs)) - 1u) & ~((1u << code_low_bits(elem_bytes)) - 1u);
}
// dictionary entries the spare bits can name: all of them (32 / 16, whatever the type), the high ones alone (8 / 4 for f32, 4 / 2 for f64)
SMH_STAGE_HD constexpr uint32_t code_values(int xs) { return 1u << (16u - code_index_bits(xs)); }
SMH_STAGE_HD constexpr uint32_t code_values_high(uint32_t elem_bytes, int xs) { return 1u << (16u - code_high_shift(elem_bytes, xs)); }
SMH_STAGE_HD constexpr uint32_t code_pack(uint32_t byte_ofs, uint32_t idx, uint32_t low, uint32_t high_shift) {
    return byte_ofs | (idx & ((1u << low) - 1u)) | ((idx >> low) << high_shift);
}
SMH_STAGE_HD constexpr uint32_t code_ofs(uint32_t c, uint32_t elem_bytes, int xs) { return c & code_ofs_mask(elem_bytes, xs); }
SMH_STAGE_HD constexpr uint32_t code_value(uint32_t c, uint32_t elem_bytes, int xs) {
    return (c & ((1u << code_low_bits(elem_bytes)) - 1u)) | ((c >> code_high_shift(elem_bytes, xs)) << code_low_bits(elem_bytes));
}
SMH_STAGE_HD constexpr uint32_t code_value_high(uint32_t c, uint32_t elem_bytes, int xs) { return c >> code_high_shift(elem_bytes, xs); }

// THE TILE MAP.  Workgroups 8 k + g share XCD g's L2: XCD g takes a contiguous run of the launch's tiles (a bijection).  The per-tile
// kernels run tile first + (blockIdx.x >> 3), the persistent one splits [first, first + count) among the XCD's workgroups.
struct XcdRun {
    uint64_t first, count;
};
SMH_STAGE_HD XcdRun xcd_run(uint64_t n_tiles, uint64_t xcd) {
    const uint64_t q = n_tiles >> 3, rm = n_tiles & 7;
    XcdRun r;
    r.first = xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q;
    r.count = q + (xcd < rm ? 1u : 0u);
    return r;
}

#if defined(__HIPCC__)
// products rounded, then added to the row's sum with a rounded add each: the reference's `sum += x * val`, whatever the contraction flags
__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
#endif

}  // namespace stage
}  // namespace smh
