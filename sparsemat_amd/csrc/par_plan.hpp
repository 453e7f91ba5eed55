// par_plan.hpp -- the arithmetic of a row partition: which rows a block owns, what every exchange moves, which rows run beside it.
// Host only: nothing of the GPU runtime or of RCCL is included, so the header compiles and is tested as a program of its own
// (tests/test_par_plan_on_host.py).  par.hip, par_step.hip and the plan entry points call it; no copy of the arithmetic lives elsewhere.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/sparsemat_hip.h"  // SMH_EXCHANGE_*

namespace smh {
namespace plan {

// Which rows a block owns.  split == NULL: the reference's arithmetic -- R = n_rows / n_blocks (sparsemat_par.rs:21), block k owns
// [k R, (k + 1) R), the last one also the remainder.  split != NULL (n_blocks + 1 ascending rows, split[0] = 0, split[n_blocks] =
// n_rows): block k owns [split[k], split[k + 1]) -- SURVEY 8e's "nnz-balanced split points ... for skewed matrices".
struct Part {
    size_t n_blocks, n_rows;
    const size_t *split;
    const uint8_t *needs; const uint32_t *lo, *hi;  // the blocks' column intervals: block q references [lo[q], hi[q]] when needs[q]
};

inline void block_rows(const Part &pt, size_t k, size_t *r0, size_t *r1) {
    if (pt.split) { *r0 = pt.split[k]; *r1 = pt.split[k + 1]; return; }
    const size_t rpb = pt.n_rows / pt.n_blocks;  // sparsemat_par.rs:21
    *r0 = k * rpb;
    *r1 = k + 1 == pt.n_blocks ? pt.n_rows : (k + 1) * rpb;  // the last block takes the remainder
}

// the block that owns `row` and the row's id inside it (the inverse of block_rows; a row past the end belongs to the last block)
inline void block_of_row(const Part &pt, size_t row, size_t *block, size_t *local) {
    if (pt.split) {  // a split table: the last block whose first row is <= row
        size_t lo = 0, hi = pt.n_blocks;
        while (hi - lo > 1) {
            const size_t mid = (lo + hi) / 2;
            if (pt.split[mid] <= row) lo = mid; else hi = mid;
        }
        *block = lo;
        *local = row - pt.split[lo];
        return;
    }
    const size_t rpb = pt.n_rows / pt.n_blocks;
    size_t k = row / rpb;  // sparsemat_par.rs:32, clamped to the last block instead of one past it
    if (k > pt.n_blocks - 1) k = pt.n_blocks - 1;
    *block = k;
    *local = row - k * rpb;
}

// the part of block src's slice that block q's columns reference (empty: *a == *e == 0)
inline void recv_range(const Part &pt, size_t q, size_t src, size_t *a, size_t *e) {
    *a = *e = 0;
    if (q == src || !pt.needs[q]) return;
    size_t s0, s1;
    block_rows(pt, src, &s0, &s1);
    const size_t x0 = pt.lo[q] > s0 ? pt.lo[q] : s0, x1 = (size_t)pt.hi[q] + 1 < s1 ? (size_t)pt.hi[q] + 1 : s1;
    if (x0 < x1) { *a = x0; *e = x1; }
}

inline void plan_summary(const Part &pt, int *auto_mode, size_t *max_recv) {
    size_t worst = 0;
    for (size_t q = 0; q < pt.n_blocks; ++q) {
        size_t got = 0;
        for (size_t src = 0; src < pt.n_blocks; ++src) {
            size_t a, e;
            recv_range(pt, q, src, &a, &e);
            got += e - a;
        }
        worst = got > worst ? got : worst;
    }
    if (max_recv) *max_recv = worst;
    if (auto_mode) *auto_mode = pt.n_blocks <= 1 ? SMH_EXCHANGE_NONE : (worst * 2 < pt.n_rows ? SMH_EXCHANGE_WINDOW : SMH_EXCHANGE_ALLGATHER);
}

// nnz-balanced boundaries: block k starts at the first row whose entries begin at or beyond k nnz / n_blocks (every block keeps at
// least one row)
inline void split_by_nnz(size_t n_blocks, size_t n_rows, const uint32_t *off, std::vector<size_t> &split) {
    split.assign(n_blocks + 1, 0);
    const uint64_t nnz = (uint64_t)off[n_rows] - off[0];
    for (size_t k = 1; k < n_blocks; ++k) {
        const uint64_t want = (uint64_t)off[0] + nnz * k / n_blocks;
        size_t lo = 0, hi = n_rows;  // first row r with off[r] >= want
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if (off[mid] < want) lo = mid + 1; else hi = mid;
        }
        size_t r = lo;
        if (r < split[k - 1] + 1) r = split[k - 1] + 1;
        if (r > n_rows - (n_blocks - k)) r = n_rows - (n_blocks - k);
        split[k] = r;
    }
    split[n_blocks] = n_rows;
}

// which rule of a split table broke, and at which block (the caller words the message)
enum class SplitFault { None, Ends, Descends };
inline SplitFault check_split(size_t n_blocks, size_t n_rows, const size_t *split, size_t *block) {
    if (split[0] != 0 || split[n_blocks] != n_rows) return SplitFault::Ends;
    for (size_t k = 0; k < n_blocks; ++k)
        if (split[k + 1] < split[k]) { *block = k; return SplitFault::Descends; }
    return SplitFault::None;
}

// ---- interior rows: the rows of a block that neither feed a window exchange nor need it ---------------------------------------
constexpr size_t kTileRows = 256;  // the interior is found by tiles of this many rows (the K1s tile)

// the tiles of block `me`, whose rows begin at r0, that hold a row another block references: dirty[t] = 1
inline void mark_referenced_tiles(const Part &pt, size_t me, size_t r0, uint8_t *dirty) {
    for (size_t q = 0; q < pt.n_blocks; ++q) {
        size_t a, e;
        recv_range(pt, q, me, &a, &e);
        if (a < e)
            for (size_t t = (a - r0) / kTileRows; t <= (e - 1 - r0) / kTileRows; ++t) dirty[t] = 1;
    }
}

// the longest run of clean tiles [*t0, *t1) (the first of equally long ones; *t0 == *t1: none)
inline void longest_clean_run(const uint8_t *dirty, size_t n_tiles, size_t *t0, size_t *t1) {
    size_t best0 = 0, best1 = 0, run0 = 0;
    for (size_t t = 0; t <= n_tiles; ++t) {
        if (t == n_tiles || dirty[t]) {
            if (t - run0 > best1 - best0) { best0 = run0; best1 = t; }
            run0 = t + 1;
        }
    }
    *t0 = best0;
    *t1 = best1;
}

// the interior [in0, in1) of a block of n_loc rows as a kernel that is launched by runs of `gran` rows can take it: [*a, *e), never
// outside [in0, in1); empty (*a == *e == 0) when nothing is left or when it would be the whole block (the product is then not split)
inline void round_interior(size_t in0, size_t in1, size_t n_loc, size_t gran, size_t *a, size_t *e) {
    *a = *e = 0;
    if (in1 <= in0 || gran == 0) return;
    const size_t lo = (in0 + gran - 1) / gran * gran, hi = in1 == n_loc ? n_loc : in1 / gran * gran;
    if (lo < hi && (lo > 0 || hi < n_loc)) { *a = lo; *e = hi; }
}

}  // namespace plan
}  // namespace smh
