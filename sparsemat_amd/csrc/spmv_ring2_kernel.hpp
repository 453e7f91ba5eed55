// spmv_ring2_kernel.hpp -- K1r, the software-pipelined ring kernel: its device helpers and the kernel templates.  Included by the
// sources that instantiate them (spmv_ring2.hip: the three-body and REGK forms; spmv_ring2_allreg.hip: the all-regular form),
// so that the two sets of instantiations compile side by side.
//
// Profile of the first K1r body (profiles/r01_pmc_sq_ring_v1.json): waves are parked on memory 81 % of
// their cycles and every wave alternates "issue 8 KiB of loads -> wait -> reduce", so the bytes in
// flight per CU sag while a wave computes.  This body keeps every wave's memory queue primed:
//
//   unit  = SB steps x (64/LANES) rows of one wave (LANES 8: 4 steps x 8 rows = 32 rows, 8 KiB of
//           columns+values)
//   per iteration, in program order (vmcnt retires in order, so older loads must be the ones needed
//   first):   offsets(unit+2)  ->  chunk loads(unit+1)  ->  consume(unit)
//   i.e. row offsets are fetched two units ahead (one coalesced load per unit, fanned out to the lane
//   groups with ds_bpermute), the 16-B column/value chunks one unit ahead, and the LDS gathers / FMAs /
//   butterfly / transposed coalesced store of the current unit run under the next unit's HBM latency.
//   Steady state is straight-line code (no branch between issue and consume), so hipcc's counted
//   s_waitcnt vmcnt(N) leaves exactly the next unit's loads in flight.
//   All chunk loads are unconditional and branch-free: addresses are clamped to the last whole chunk
//   that is safe to read, entries outside the row are masked with selects (never multiplied in: LDS
//   garbage may be NaN), and the <= 3 entries of an unpadded array's final partial chunk are added by
//   a one-thread fix-up kernel (in storage order: they are the last entries of their rows).
//   A REGULAR phase (ring gathers, every row L > 0 entries long: RingPlan::reg_len) does not stream its row offsets at all: they
//   are off[row_begin] + i * L, computed where the other body loads them (phase_rows<..., REG>, in the REGK form of the kernel).
#pragma once
#include "internal.hpp"
#include "ring_col12.hpp"
#include "ring_val24.hpp"

namespace smh {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// The ring holds kRingEntries columns for either value type (the plan does not depend on T):
//   f32: 64 KiB  -> 512-thread blocks, two resident per CU;
//   f64: 128 KiB -> 1024-thread blocks, one resident per CU (same 16 waves per CU, <= 128 VGPRs).
// LDS is dynamic (above the 64 KiB static limit for f64).
// RING = columns the ring holds: 16384 by default; f32 matrices whose rows do not fit that but fit 32768 take the
// 128 KiB / 1024-thread configuration too (chosen by the plan builder's caller).
#ifndef SMH_RING2_THREADS64
#define SMH_RING2_THREADS64 1024
#endif
template <typename T, int RING> struct Ring2Cfg {
    static constexpr bool kBig = (size_t)RING * sizeof(T) > 65536;  // 128 KiB of LDS: one workgroup per CU
    static constexpr int kThreads = kBig ? (sizeof(T) == 8 ? SMH_RING2_THREADS64 : 1024) : 512;
    // wavefronts per SIMD the register budget is sized for: the CU's resident workgroups' wavefronts over its 4 SIMDs
    static constexpr int kWavesPerSimd = (kBig ? 1 : 2) * (kThreads / 64) / 4;
};
#ifndef SMH_RING2_SB
#define SMH_RING2_SB 2
#endif
constexpr int kRing2SB = SMH_RING2_SB;
#ifndef SMH_RING2_SB64
#define SMH_RING2_SB64 1
#endif
// steps per unit: two units x SB x 32 B per lane live in VGPRs
// Addressing A/B (same box, interleaved runs): 32-bit byte offsets (saddr form, would also need a < 2^30
// entries-per-phase guard) gave 0.465 vs 0.465 ms on C2 and 2.89 vs 2.76 ms on the 512^3 Laplacian against
// 64-bit offsets -- no gain, so the guard-free 64-bit form is the default.
#ifndef SMH_RING2_SADDR
#define SMH_RING2_SADDR 0
#endif
#if SMH_RING2_SADDR
#define SMH_R2_OFF(rel, size) ((size_t)((rel) * (size)))
#else
#define SMH_R2_OFF(rel, size) ((size_t)(rel) * (size))
#endif

template <typename T, int NCH>
struct Unit {
    uint32_t o0, o1;  // lane L: off[base+L], off[base+L+1] (rows clamped to the phase end)
    uint32_t c[NCH][4];
    T v[NCH][4];
};

// WHICH entries of a pass (4 LANES consecutive entry slots of a row, starting on the 4-entry grid) lane j of the row's group takes.
//   f32: slots 4j .. 4j+3 -- 16 bytes of values per lane, one load instruction covers 16 LANES contiguous bytes per row.
//   f64: slots 2j, 2j+1 and 2 LANES + 2j, 2 LANES + 2j + 1 -- TWO 16-byte loads per lane, each of which covers 16 LANES contiguous bytes
//        per row (LANES 8: a whole 128-byte line).  Round 3 gave an f64 lane 32 contiguous bytes: each of its two load instructions
//        then touched every line of the row but used half of it, and the kernel ran at 4.9 TB/s where the f32 one reaches 6.2; with
//        whole lines per instruction 0.67-0.70 -> 0.58-0.60 ms on the headline shape (profiles/r04_k1r_f64_line_loads.log).
template <typename T, int LANES>
__device__ __forceinline__ uint32_t lane_pos(uint32_t j, int q) {
    if constexpr (sizeof(T) == 8) return q < 2 ? 2u * j + (uint32_t)q : 2u * LANES + 2u * j + (uint32_t)(q - 2);
    else return 4u * j + (uint32_t)q;
}

// colp/valp are wave-uniform (SGPR) base pointers of the phase's first chunk, pass_rel the 32-bit element offset of the pass from
// it: hipcc emits the saddr form `global_load_dwordx4 v, v_off, s[base]`, one address VGPR per load.  Every address is clamped to the
// last piece that is safe to read (last_rel: the last whole 4-entry chunk of the arrays): lanes without work re-read a valid piece,
// which the caller masks.
// CF, the column form a phase streams:
//   kColU32: colp points into the 32-bit column array
//   kCol16:  ... into the 16-bit column array (the low halves of the columns: all a ring phase needs, since the ring slot of a
//            column is `column mod 16384`) -- 4 columns are then 8 bytes (f32: one load; f64: two of 4 bytes)
//   kCol12:  ... into the byte array of the compact form (ring_col12.hpp; f32 on the 16384-slot ring), and hdrp into its u16
//            chunk headers -- 4 columns are 4 + 2 bytes, decoded where they are used (chunk_slots)
//   kRec16:  ... into the 16-byte chunk records of ring_val24.hpp: a chunk's four VALUES as 24-bit integers (three dwords) and, in
//            the fourth dword, what kCol12's byte array holds for the chunk; hdrp as for kCol12.  One load brings values and low
//            column bytes, the value array is not read: 4 + 2 bytes per 4 entries less than kCol12 (f32, 16384-slot ring,
//            matrices whose values all fit the code)
enum : int { kColU32 = 0, kCol16 = 1, kCol12 = 2, kRec16 = 3 };
constexpr bool has_headers(int cf) { return cf == kCol12 || cf == kRec16; }  // the forms that take ring slots from ring_col12.hpp's code
struct ColStream {
    const void *colp;          // wave-uniform base of the phase's first chunk in the array of its form
    const uint16_t *hdrp;      // kCol12, kRec16: ... and in the chunk headers
    const uint16_t *table;     // kCol12, kRec16: the triple table (in LDS)
    const u32x2 *escapes;      // kCol12, kRec16: the side table
    float scale;               // kRec16: 2^E, what the 24-bit integers are multiples of
};
template <typename T, int CF, int LANES>
__device__ __forceinline__ void load_chunk_nb(const ColStream &cs, const T *__restrict__ valp, uint32_t pass_rel, uint32_t j,
                                              uint32_t last_rel, uint32_t (&c)[4], T (&v)[4]) {
    const void *colp = cs.colp;
    if constexpr (sizeof(T) == 4) {
        uint32_t rel = pass_rel + 4u * j;
        rel = rel < last_rel ? rel : last_rel;
        if constexpr (CF == kRec16) {  // v[0..2]: the record's three value dwords (bits, decoded where they are used), c[0] / c[1] as kCol12
            const u32x4 r = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(
                reinterpret_cast<const char *>(colp) + SMH_R2_OFF(rel, 4u)));
            // (scalars first: __builtin_bit_cast applied to a vector's element reads the vector's first bytes, whichever element is named)
            const uint32_t w0 = r.x, w1 = r.y, w2 = r.z;
            c[0] = r.w;
            c[1] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(cs.hdrp) + (SMH_R2_OFF(rel, 1u) >> 1)));
            v[0] = __uint_as_float(w0); v[1] = __uint_as_float(w1); v[2] = __uint_as_float(w2);
            v[3] = 0.0f;  // (never read)
            return;
        } else if constexpr (CF == kCol12) {  // c[0]: the chunk's four low bytes (or its side-table index), c[1]: its header
            c[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(colp) + SMH_R2_OFF(rel, 1u)));
            c[1] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(cs.hdrp) + (SMH_R2_OFF(rel, 1u) >> 1)));
        } else if constexpr (CF == kCol16) {  // kept packed: c[0], c[1] hold two columns each (unpacked where they are used, see chunk_slots)
            const u32x2 cc = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(
                reinterpret_cast<const char *>(colp) + SMH_R2_OFF(rel, 2u)));
            c[0] = cc.x; c[1] = cc.y;  // (unpacking here instead measured the same: 0.343-0.345 ms either way)
        } else {
            const u32x4 cc = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(
                reinterpret_cast<const char *>(colp) + SMH_R2_OFF(rel, 4u)));
            c[0] = cc.x; c[1] = cc.y; c[2] = cc.z; c[3] = cc.w;
        }
        const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(
            reinterpret_cast<const char *>(valp) + SMH_R2_OFF(rel, 4u)));
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
        // two pieces of 2 entries (even positions; the last readable one is last_rel + 2)
        uint32_t e0 = pass_rel + 2u * j, e1 = pass_rel + 2u * LANES + 2u * j;
        e0 = e0 < last_rel + 2u ? e0 : last_rel + 2u;
        e1 = e1 < last_rel + 2u ? e1 : last_rel + 2u;
        static_assert(!has_headers(CF), "the compact column form and the chunk records are f32 forms");
        if constexpr (CF == kCol16) {
            c[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(colp) + SMH_R2_OFF(e0, 2u)));
            c[1] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(colp) + SMH_R2_OFF(e1, 2u)));
        } else {
            const u32x2 c0 = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(reinterpret_cast<const char *>(colp) + SMH_R2_OFF(e0, 4u)));
            const u32x2 c1 = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(reinterpret_cast<const char *>(colp) + SMH_R2_OFF(e1, 4u)));
            c[0] = c0.x; c[1] = c0.y; c[2] = c1.x; c[3] = c1.y;
        }
        const f64x2 a = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(reinterpret_cast<const char *>(valp) + SMH_R2_OFF(e0, 8u)));
        const f64x2 b = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(reinterpret_cast<const char *>(valp) + SMH_R2_OFF(e1, 8u)));
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    }
}

// ring slots of a chunk's four entries: column mod kRingEntries, from the u32 columns, from the packed 16-bit pairs or from
// the compact form.  There the escape is a wave-uniform branch that almost no wave takes (the form is only chosen by itself
// for matrices with at most one escaped chunk in 1024): the lanes whose chunk escaped fetch its 8 bytes of true slots.
template <int CF, int RING>
__device__ __forceinline__ void chunk_slots(const uint32_t (&c)[4], const ColStream &cs, uint32_t (&slot)[4]) {
    constexpr uint32_t MASK = RING - 1;
    if constexpr (has_headers(CF)) {
        static_assert(RING == (int)col12::kSlots, "the compact column form holds slots of the 16384-slot ring");
        col12::decode_chunk(c[1], c[0], cs.table, slot);
        const bool escaped = col12::is_escape(c[1]);
        if (__builtin_amdgcn_ballot_w64(escaped) != 0) {
            if (escaped) {
                const u32x2 e = cs.escapes[c[0]];
                col12::unpack_escape(e.x, e.y, slot);
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (CF == kCol16) slot[q] = (q & 1) ? ((c[q >> 1] >> 16) & MASK) : (c[q >> 1] & MASK);
            else slot[q] = c[q] & MASK;
        }
    }
}

__device__ __forceinline__ float r2_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// a chunk's four values as the unit holds them: themselves, or (kRec16) the three dwords of 24-bit integers they are decoded from --
// (float)k * 2^E gives the very bits the value array holds (ring_val24.hpp; the form is only built for matrices where it does)
template <typename T, int CF>
__device__ __forceinline__ void chunk_values(const T (&v)[4], const ColStream &cs, T (&a)[4]) {
    if constexpr (CF == kRec16) {
        static_assert(sizeof(T) == 4, "the chunk records are an f32 form");
        val24::decode_chunk(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), cs.scale, a);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = v[q];
    }
}
__device__ __forceinline__ double r2_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename T, int NCH>
__device__ __forceinline__ void load_offsets(Unit<T, NCH> &u, const uint32_t *__restrict__ off, uint64_t base,
                                             uint64_t row_end, uint32_t lane) {
    uint64_t r0 = base + lane, r1 = base + lane + 1;
    r0 = r0 < row_end ? r0 : row_end;
    r1 = r1 < row_end ? r1 : row_end;
    u.o0 = off[r0];
    u.o1 = off[r1];
}

// ... of a REGULAR phase (rows [rb, re] all L entries apart, e0 = off[rb]: RingPlan::reg_len): the same two values without the
// loads.  32-bit arithmetic is exact: every offset is <= nnz < 2^32.
template <typename T, int NCH>
__device__ __forceinline__ void regular_offsets(Unit<T, NCH> &u, uint32_t e0, uint32_t L, uint64_t rb, uint64_t base, uint64_t row_end,
                                                uint32_t lane) {
    // wave-uniform: the unit's first row within the phase (clamped to its end) and the rows from there to the end -- nothing can wrap
    const uint32_t n = (uint32_t)(row_end - rb), d = base - rb < n ? (uint32_t)(base - rb) : n, left = n - d;
    u.o0 = e0 + (d + (lane < left ? lane : left)) * L;
    u.o1 = e0 + (d + (lane + 1u < left ? lane + 1u : left)) * L;
}

// row bounds of (step t, this lane's group), limited to the entries the kernel may touch
template <int LANES>
__device__ __forceinline__ void row_bounds(uint32_t o0, uint32_t o1, int t, uint32_t lane, uint32_t nnz_lim,
                                           uint32_t &s, uint32_t &e) {
    if constexpr (LANES == 1) {  // one lane per row: the lane already holds its own row's offsets
        s = o0;
        e = o1;
    } else {
        constexpr int RPS = kWave / LANES;
        const int src = t * RPS + (int)(lane / LANES);
        s = (uint32_t)__shfl((int)o0, src, kWave);
        e = (uint32_t)__shfl((int)o1, src, kWave);
    }
    s = s < nnz_lim ? s : nnz_lim;
    e = e < nnz_lim ? e : nnz_lim;
}

// A lane group covers 4*LANES*CH entry slots of its row per pass: chunk (ch, j) = slots [4*(ch*LANES+j), +4)
template <typename T, int LANES, int CH, int SB, int CF>
__device__ __forceinline__ void issue_unit(Unit<T, SB * CH> &u, const ColStream &cs,
                                           const T *__restrict__ valp, uint32_t kb, uint32_t nnz_lim, uint32_t last_rel,
                                           uint32_t lane) {
    const uint32_t j = lane % LANES;
#pragma unroll
    for (int t = 0; t < SB; ++t) {
        uint32_t s, e;
        row_bounds<LANES>(u.o0, u.o1, t, lane, nnz_lim, s, e);
        s = s > kb ? s : kb;  // (only rows past the arrays' readable end are below kb: they are empty)
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            // (lanes without work re-read a valid piece: clamped inside, masked when consumed)
            load_chunk_nb<T, CF, LANES>(cs, valp, (s & ~3u) - kb + 4u * (uint32_t)(ch * LANES), j, last_rel, u.c[t * CH + ch], u.v[t * CH + ch]);
        }
    }
}

// DOT (SparseMatrix::inner_prod, sparsematrix.rs:161-171): `y` then holds lhs, nothing is stored, and every lane adds
// lhs[row] * (A x)[row] of the rows it would have stored to its *dacc -- of the rows that hold entries: the reference reads lhs[i]
// inside the entry loop, so what lhs holds on a row without entries (NaN, Inf) never reaches the sum.  Lane L < RU holds the
// offsets of row base + L, the row whose sum it keeps, in u.o0 / u.o1 (load_offsets, regular_offsets): no load is added.  With
// finite data nothing changes: dacc starts at +0 and never becomes -0, and lhs * (+0) = +-0 added to it leaves its bits.
template <typename T, int LANES, int CH, int SB, int GM, int CF, int RING, bool DOT = false>
__device__ __forceinline__ void consume_unit(const Unit<T, SB * CH> &u, uint64_t base, uint64_t row_end,
                                             const ColStream &cs, const T *__restrict__ valp,
                                             const T *__restrict__ x, const T *ring, T *__restrict__ y, uint32_t kb,
                                             uint32_t nnz_lim, uint32_t last_rel, uint32_t lane, T *dacc = nullptr) {
    constexpr int RPS = kWave / LANES;
    const uint32_t j = lane % LANES;
    T out = T(0);
#pragma unroll
    for (int t = 0; t < SB; ++t) {
        uint32_t s, e;
        row_bounds<LANES>(u.o0, u.o1, t, lane, nnz_lim, s, e);
        s = s > kb ? s : kb;
        e = e > s ? e : s;
        const uint32_t sa = s & ~3u;      // chunk grid is anchored at element 0
        const uint32_t lo = s - sa;       // 0..3: entries of the first chunk that belong to the previous row
        const uint32_t len = e - sa;      // row end relative to the aligned start
        T sum = T(0);
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            uint32_t slot[4];
            if constexpr (GM == 1) chunk_slots<CF, RING>(u.c[t * CH + ch], cs, slot);
            T a[4];
            chunk_values<T, CF>(u.v[t * CH + ch], cs, a);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t rel = 4u * (uint32_t)(ch * LANES) + lane_pos<T, LANES>(j, q);
                const bool in = rel >= lo && rel < len;
                T xv;
                // (round 4, a build that is wrong on purpose: every lane gathering its OWN slot -- no bank conflicts -- ran exactly as
                // fast, 0.699 against 0.698 ms on f64 and 0.353 against 0.353 on f32: the random LDS gathers are not what bounds K1r)
                if constexpr (GM == 1) xv = ring[slot[q]];
                else if constexpr (GM == 2) xv = __builtin_nontemporal_load(&x[in ? u.c[t * CH + ch][q] : 0u]);
                else xv = x[in ? u.c[t * CH + ch][q] : 0u];
                const T f = r2_fma(a[q], xv, sum);
                sum = in ? f : sum;
            }
        }
        // rows longer than one pass of the lane group (rare; not pipelined)
        for (uint32_t pass = 4u * (uint32_t)(CH * LANES); pass + lane_pos<T, LANES>(j, 0) < len; pass += 4u * LANES) {
            uint32_t cc[4];
            T vv[4];
            load_chunk_nb<T, CF, LANES>(cs, valp, sa - kb + pass, j, last_rel, cc, vv);
            uint32_t slot[4];
            if constexpr (GM == 1) chunk_slots<CF, RING>(cc, cs, slot);
            T a[4];
            chunk_values<T, CF>(vv, cs, a);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = pass + lane_pos<T, LANES>(j, q) < len;
                T xv;
                if constexpr (GM == 1) xv = ring[slot[q]];
                else if constexpr (GM == 2) xv = __builtin_nontemporal_load(&x[in ? cc[q] : 0u]);
                else xv = x[in ? cc[q] : 0u];
                const T f = r2_fma(a[q], xv, sum);
                sum = in ? f : sum;
            }
        }
        if constexpr (LANES == 1) {
            out = sum;
        } else {
#pragma unroll
            for (int o = LANES / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, kWave);
            // transpose: lane L keeps the sum of the unit's row L (held by every lane of group L % RPS in step L / RPS)
            const T got = __shfl(sum, (int)((lane % RPS) * LANES), kWave);
            out = ((int)(lane / RPS) == t) ? got : out;
        }
    }
    const uint64_t row = base + lane;
    if constexpr (DOT) {
        if (lane < (uint32_t)(SB * RPS) && row < row_end && u.o1 != u.o0) *dacc = r2_fma(y[row], out, *dacc);
    } else {
        if (lane < (uint32_t)(SB * RPS) && row < row_end) y[row] = out;
    }
}

// cols: the arrays of the column form CF from their first element (colp: the 32-bit columns, the 16-bit ones or the compact form's bytes)
// REG: the phase is regular with row length L (RingPlan::reg_len): the units' offsets are computed, the offset array is read for
// off[rb] alone, and nothing the chunk addresses are made of waits for a load
// WAVES: the wavefronts of the workgroup (a wave's units are WAVES units apart)
template <typename T, int LANES, int CH, int GM, int CF, int RING, bool DOT = false, bool REG = false,
          int WAVES = Ring2Cfg<T, RING>::kThreads / kWave>
__device__ __forceinline__ void phase_rows(const uint32_t *__restrict__ off, const ColStream &cols,
                                           const T *__restrict__ val, const T *__restrict__ x, const T *ring,
                                           T *__restrict__ y, uint64_t rb, uint64_t re, uint32_t nnz_lim,
                                           uint64_t last_chunk, uint32_t wave, uint32_t lane, T *dacc = nullptr, uint32_t L = 0) {
    constexpr int STEPS = LANES;
    constexpr int SBMAX = sizeof(T) == 8 ? SMH_RING2_SB64 : kRing2SB;  // f64 chunks take 12 VGPRs: one step per unit (two: A/B in round 4)
    constexpr int SB = STEPS < SBMAX ? STEPS : SBMAX;
    constexpr int RU = SB * (kWave / LANES);                 // rows per unit
    constexpr uint64_t STRIDE = (uint64_t)WAVES * RU;        // rows between two units of a wave
    uint64_t base = rb + (uint64_t)wave * RU;
    if (base >= re) return;
    // 32-bit addressing inside the phase: everything is relative to the phase's first (aligned) entry
    const uint32_t e0 = __builtin_amdgcn_readfirstlane(off[rb]);
    uint32_t kb = e0 & ~3u;
    kb = kb < (uint32_t)last_chunk ? kb : (uint32_t)last_chunk;
    const uint32_t last_rel = (uint32_t)last_chunk - kb;
    ColStream cs = cols;  // ... from the phase's first chunk (kb is a multiple of 4: kb / 4 chunks)
    cs.colp = reinterpret_cast<const char *>(cols.colp) + (size_t)kb * (CF == kCol12 ? 1u : CF == kCol16 ? 2u : 4u);  // (kRec16: 16 bytes per 4 entries)
    if constexpr (has_headers(CF)) cs.hdrp = cols.hdrp + (kb >> 2);
    const T *valp = val + kb;
    if constexpr (REG) {
        Unit<T, SB * CH> A, B;
        regular_offsets(A, e0, L, rb, base, re, lane);
        regular_offsets(B, e0, L, rb, base + STRIDE, re, lane);
        // the loop of the loading body below without the unit N: the offsets of the unit after next are computed where that body
        // copies them.  (Three units in rotation, two of them in flight -- the addresses wait for no load, so it is cheap --
        // measured no better: DESIGN.md Appendix A.)
        issue_unit<T, LANES, CH, SB, CF>(A, cs, valp, kb, nnz_lim, last_rel, lane);
        for (;;) {
            if (base + STRIDE >= re) {
                consume_unit<T, LANES, CH, SB, GM, CF, RING, DOT>(A, base, re, cs, valp, x, ring, y, kb, nnz_lim, last_rel, lane, dacc);
                break;
            }
            issue_unit<T, LANES, CH, SB, CF>(B, cs, valp, kb, nnz_lim, last_rel, lane);
            consume_unit<T, LANES, CH, SB, GM, CF, RING, DOT>(A, base, re, cs, valp, x, ring, y, kb, nnz_lim, last_rel, lane, dacc);
            regular_offsets(A, e0, L, rb, base + 2 * STRIDE, re, lane);
            base += STRIDE;
            if (base + STRIDE >= re) {
                consume_unit<T, LANES, CH, SB, GM, CF, RING, DOT>(B, base, re, cs, valp, x, ring, y, kb, nnz_lim, last_rel, lane, dacc);
                break;
            }
            issue_unit<T, LANES, CH, SB, CF>(A, cs, valp, kb, nnz_lim, last_rel, lane);
            consume_unit<T, LANES, CH, SB, GM, CF, RING, DOT>(B, base, re, cs, valp, x, ring, y, kb, nnz_lim, last_rel, lane, dacc);
            regular_offsets(B, e0, L, rb, base + 2 * STRIDE, re, lane);
            base += STRIDE;
        }
        return;
    }
    Unit<T, SB * CH> A, B, N;  // N: only its offsets are used (the unit after next)
    load_offsets(A, off, base, re, lane);
    load_offsets(B, off, base + STRIDE, re, lane);
    issue_unit<T, LANES, CH, SB, CF>(A, cs, valp, kb, nnz_lim, last_rel, lane);
    for (;;) {
        if (base + STRIDE >= re) {
            consume_unit<T, LANES, CH, SB, GM, CF, RING, DOT>(A, base, re, cs, valp, x, ring, y, kb, nnz_lim, last_rel, lane, dacc);
            break;
        }
        // program order = age order: offsets(+2) older than chunks(+1); both stay in flight under consume
        load_offsets(N, off, base + 2 * STRIDE, re, lane);
        issue_unit<T, LANES, CH, SB, CF>(B, cs, valp, kb, nnz_lim, last_rel, lane);
        consume_unit<T, LANES, CH, SB, GM, CF, RING, DOT>(A, base, re, cs, valp, x, ring, y, kb, nnz_lim, last_rel, lane, dacc);
        A.o0 = N.o0; A.o1 = N.o1;
        base += STRIDE;
        if (base + STRIDE >= re) {
            consume_unit<T, LANES, CH, SB, GM, CF, RING, DOT>(B, base, re, cs, valp, x, ring, y, kb, nnz_lim, last_rel, lane, dacc);
            break;
        }
        load_offsets(N, off, base + 2 * STRIDE, re, lane);
        issue_unit<T, LANES, CH, SB, CF>(A, cs, valp, kb, nnz_lim, last_rel, lane);
        consume_unit<T, LANES, CH, SB, GM, CF, RING, DOT>(B, base, re, cs, valp, x, ring, y, kb, nnz_lim, last_rel, lane, dacc);
        B.o0 = N.o0; B.o1 = N.o1;
        base += STRIDE;
    }
}

// the triple table of the compact column form, as every workgroup of a kCol12 kernel copies it into LDS
__device__ const col12::Table k_col12_table = col12::make_table();

// ... by a workgroup of THREADS threads, behind the ring; ends with a barrier.  512 threads copy one dword each.
template <typename T, int RING, int THREADS>
__device__ __forceinline__ uint16_t *copy_col12_table(unsigned char *ring_raw) {
    constexpr int kDwords = (int)(sizeof(col12::Table) / sizeof(uint32_t));
    uint16_t *table = reinterpret_cast<uint16_t *>(ring_raw + (size_t)RING * sizeof(T));
    if constexpr (THREADS == kDwords) {
        reinterpret_cast<uint32_t *>(table)[threadIdx.x] = reinterpret_cast<const uint32_t *>(k_col12_table.e)[threadIdx.x];
    } else {
        for (int i = (int)threadIdx.x; i < kDwords; i += THREADS)
            reinterpret_cast<uint32_t *>(table)[i] = reinterpret_cast<const uint32_t *>(k_col12_table.e)[i];
    }
    __syncthreads();
    return table;
}

// what a phase adds to the ring before its rows are taken: columns [load_lo, load_hi) of x (band 0) and, in a banded plan (MASK + 1
// slots per band), those of bands 1..3; between two barriers, by a workgroup of THREADS threads
template <typename T, int THREADS>
__device__ __forceinline__ void fill_ring(const RingPhase &ph, uint32_t bands, uint32_t MASK, const T *__restrict__ x, T *ring) {
    const bool more = bands == 4u && (ph.band_hi[0] > ph.band_lo[0] || ph.band_hi[1] > ph.band_lo[1] || ph.band_hi[2] > ph.band_lo[2]);
    if (ph.load_hi > ph.load_lo || more) {
        __syncthreads();  // the previous phase's gathers are done before its slots are overwritten
        for (uint64_t cidx = (uint64_t)ph.load_lo + threadIdx.x; cidx < ph.load_hi; cidx += THREADS)
            ring[cidx & MASK] = x[cidx];
        if (more) {
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k)
                for (uint64_t cidx = (uint64_t)ph.band_lo[k] + threadIdx.x; cidx < ph.band_hi[k]; cidx += THREADS)
                    ring[(k + 1u) * (MASK + 1u) + (cidx & MASK)] = x[cidx];
        }
        __syncthreads();
    }
}

// CF: what ring phases stream for their columns -- kCol16: the 16-bit column array `col16` (6 instead of 8 bytes per f32 entry);
// kCol12: the compact form `c12` (5.5 bytes; LDS then holds the ring and, behind it, the 2 KiB triple table); phases with
// global gathers need whole columns and keep reading `col`
// DOT: y holds lhs (read only) and dot_partials[blockIdx.x] = this block's share of lhs . (A x); nothing else is stored
// REGK: the kernel for plans whose phases ALL gather from the ring and of which some are regular -- reg_len[p] (RingPlan::reg_len)
// sends phase p to the body that computes its row offsets (L != 0) or to the one that loads them.  A kernel of its own and not
// a fourth body beside the other three: the bodies' registers add up (one body of the f32 headline kernel takes 76-82 VGPRs,
// the three of the other form all 128, a fourth spilled 92 bytes per lane), and these two take 97.
// kRec16 exists in the REGK form alone (91 VGPRs on the headline shape, no scratch in any instantiation): the three bodies of the
// other form spill with it in the DOT instantiations, so a plan that does not take the REGK kernel is not offered the records.
template <typename T, int LANES, int CH, int CF, int RING, bool DOT = false, bool REGK = false>
__global__ void __launch_bounds__((Ring2Cfg<T, RING>::kThreads), (Ring2Cfg<T, RING>::kWavesPerSimd))
k_spmv_ring2(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const uint16_t *__restrict__ col16, RingCol12 c12,
             const T *__restrict__ val, const T *__restrict__ x, T *__restrict__ y, uint32_t nnz_lim, uint64_t last_chunk,
             const uint32_t *__restrict__ phase_ptr, const RingPhase *__restrict__ phases, uint32_t bands,
             T *__restrict__ dot_partials, uint32_t lb0, uint32_t lb_n, const uint32_t *__restrict__ reg_len) {
    static_assert(CF != kRec16 || REGK, "the chunk records are streamed by the REGK form only");
    T dacc_v = T(0);
    T *dacc = DOT ? &dacc_v : nullptr;
    extern __shared__ __attribute__((aligned(16))) unsigned char ring_raw[];  // RING * sizeof(T) (kCol12: + the triple table), dynamic
    T *ring = reinterpret_cast<T *>(ring_raw);
    // bands == 1: one window, slot = column mod RING.  bands == 4 (banded plan, kCol16 only): band k owns slots
    // [k * S, (k + 1) * S), S = RING / 4, slot = k * S + column mod S -- which is what col16 then holds
    const uint32_t MASK = (bands == 4u ? (uint32_t)RING / 4u : (uint32_t)RING) - 1u;
    constexpr int kRing2Threads = Ring2Cfg<T, RING>::kThreads;
    const uint32_t per_xcd = gridDim.x >> 3;
    // XCD-aware: neighbours share an L2.  A launch covers the plan's row ranges [lb0, lb0 + lb_n) (all of them, or -- the
    // partitioned product, par_step.hip -- a block's boundary / interior ranges); the grid is lb_n rounded up to a multiple of 8
    const uint32_t lb_rel = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if (lb_rel >= lb_n) return;  // (whole workgroup, before any barrier)
    const uint32_t lb = lb0 + lb_rel;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t p0 = phase_ptr[lb], p1 = phase_ptr[lb + 1];
    ColStream ring_cols = {CF == kCol16 ? (const void *)col16 : (const void *)col, nullptr, nullptr, nullptr, 0.0f};
    const ColStream wide_cols = {col, nullptr, nullptr, nullptr, 0.0f};
    if constexpr (has_headers(CF)) {
        const uint16_t *table = copy_col12_table<T, RING, kRing2Threads>(ring_raw);
        ring_cols = {CF == kRec16 ? (const void *)c12.rec16 : (const void *)c12.lo8, c12.hdr, table, reinterpret_cast<const u32x2 *>(c12.escapes), c12.scale};
    }
    for (uint32_t p = p0; p < p1; ++p) {
        const RingPhase ph = phases[p];
        fill_ring<T, kRing2Threads>(ph, bands, MASK, x, ring);
        // gather mode of the phase: 1 = LDS ring, 0 = L1/L2-cached global gathers, 2 = L1-bypassing (nt) global
        // gathers for phases whose columns have no locality to keep in the 32 KiB L1
        if constexpr (REGK) {
            static_assert(CF != kColU32, "regular phases stream one of the narrow column forms");
            const uint32_t L = reg_len[p];  // wave-uniform
            if (L != 0)
                phase_rows<T, LANES, CH, 1, CF, RING, DOT, true>(off, ring_cols, val, x, ring, y, ph.row_begin, ph.row_end, nnz_lim,
                                                                 last_chunk, wave, lane, dacc, L);
            else
                phase_rows<T, LANES, CH, 1, CF, RING, DOT>(off, ring_cols, val, x, ring, y, ph.row_begin, ph.row_end, nnz_lim, last_chunk,
                                                           wave, lane, dacc);
        } else if (ph.use_ring == 1)
            phase_rows<T, LANES, CH, 1, CF, RING, DOT>(off, ring_cols, val, x, ring, y, ph.row_begin, ph.row_end, nnz_lim, last_chunk, wave,
                                                       lane, dacc);
        else if (ph.use_ring == 2)
            phase_rows<T, LANES, CH, 2, kColU32, RING, DOT>(off, wide_cols, val, x, ring, y, ph.row_begin, ph.row_end, nnz_lim, last_chunk, wave,
                                                          lane, dacc);
        else
            phase_rows<T, LANES, CH, 0, kColU32, RING, DOT>(off, wide_cols, val, x, ring, y, ph.row_begin, ph.row_end, nnz_lim, last_chunk, wave,
                                                          lane, dacc);
    }
    if constexpr (DOT) {  // fixed order: lanes (butterfly), waves (index order) -- bitwise reproducible
        __shared__ T s_dot[kRing2Threads / kWave];
        T d = dacc_v;
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) d += __shfl_down(d, o, kWave);
        if (lane == 0) s_dot[wave] = d;
        __syncthreads();
        if (threadIdx.x == 0) {
            T t = T(0);
            for (int w = 0; w < kRing2Threads / kWave; ++w) t += s_dot[w];
            dot_partials[blockIdx.x] = t;
        }
    }
}

// The ALL-REGULAR form: the kernel for plans whose phases are ALL regular ring phases (RingPlan::reg_all) on the single-window ring,
// without DOT.  Its phase loop has the REG body alone, which takes 69-76 VGPRs where the two bodies of the REGK form take 91-97:
// workgroups of THREADS = 768 threads, two of them per CU like the 512-thread ones (the same 66 KiB of LDS each), are 6 wavefronts
// per SIMD instead of 4.  A row is taken by the same lanes with the same chunks in the same order, whichever wave it falls to: y is
// the REGK form's bit for bit.  reg_len[p] of a phase without rows is 0 (k_ring_regular): the body returns for it before it reads
// anything, `base >= re`.
template <typename T, int LANES, int CH, int CF, int RING, int THREADS>
__global__ void __launch_bounds__(THREADS, 2 * (THREADS / kWave) / 4)
k_spmv_ring2_allreg(const uint32_t *__restrict__ off, const uint16_t *__restrict__ col16, RingCol12 c12, const T *__restrict__ val,
                    const T *__restrict__ x, T *__restrict__ y, uint32_t nnz_lim, uint64_t last_chunk,
                    const uint32_t *__restrict__ phase_ptr, const RingPhase *__restrict__ phases, uint32_t lb0, uint32_t lb_n,
                    const uint32_t *__restrict__ reg_len) {
    static_assert(CF != kColU32, "regular phases stream one of the narrow column forms");
    static_assert(THREADS % (4 * kWave) == 0, "the workgroup's wavefronts divide over the four SIMDs");
    extern __shared__ __attribute__((aligned(16))) unsigned char ring_raw[];  // RING * sizeof(T) (kCol12, kRec16: + the triple table)
    T *ring = reinterpret_cast<T *>(ring_raw);
    const uint32_t per_xcd = gridDim.x >> 3;  // (row ranges to workgroups as in k_spmv_ring2)
    const uint32_t lb_rel = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if (lb_rel >= lb_n) return;  // (whole workgroup, before any barrier)
    const uint32_t lb = lb0 + lb_rel;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t p0 = phase_ptr[lb], p1 = phase_ptr[lb + 1];
    ColStream ring_cols = {(const void *)col16, nullptr, nullptr, nullptr, 0.0f};
    if constexpr (has_headers(CF)) {
        const uint16_t *table = copy_col12_table<T, RING, THREADS>(ring_raw);
        ring_cols = {CF == kRec16 ? (const void *)c12.rec16 : (const void *)c12.lo8, c12.hdr, table, reinterpret_cast<const u32x2 *>(c12.escapes), c12.scale};
    }
    for (uint32_t p = p0; p < p1; ++p) {
        const RingPhase ph = phases[p];
        fill_ring<T, THREADS>(ph, 1u, (uint32_t)RING - 1u, x, ring);
        phase_rows<T, LANES, CH, 1, CF, RING, false, true, THREADS / kWave>(off, ring_cols, val, x, ring, y, ph.row_begin, ph.row_end, nnz_lim,
                                                                            last_chunk, wave, lane, nullptr, reg_len[p]);
    }
}

}  // namespace smh
