// matupdate.hip -- element access of a SparseMatCRS on the device, gfx950: a batched SparseMatrix::get (sparsemat_crs.rs:136-142)
// and a batched stream of `set` / `add_to` calls (sparsematrix.rs:224-233) on an existing handle.
//
// What it replaces.  `m.add_to(i, j, v)` is `*m.get_mut(i, j) += v`, `m.set(i, j, v)` is `*m.get_mut(i, j) = v`; get_mut is
// find_index (the FIRST match in row i, sparsemat_crs.rs:54-67) or else push, which inserts at the START of the row (:71-92).  On
// the host that is a row scan per call plus a Vec::insert per new entry.  For a handle with rows the result of a whole stream is
// fixed in closed form (tests/update_model.py restates it):
//   * row i = its new columns in REVERSE order of first appearance among the stream's operations on row i, then m's row i;
//   * an operation whose (row, column) exists in m's row goes to the first occurrence; a new (row, column) is one new entry;
//   * every target's value is the left fold of its operations in stream order, from m's value or from +0 for a new entry
//     (add_to: acc + v, one rounding; set: v);
//   * n_rows = max(m.n_rows, 1 + largest row of any operation), n_cols = max(m.n_cols, 1 + largest column of a new entry).
// Device formulation (integer structure and values bit for bit, no float atomics: the fold order is the contract):
//   1. lookup: every operation's target in m -- the first match in its row, or absent (rows past the end are absent without a
//      load).  Rows are unsorted and may repeat columns, so this is a scan of the row: one thread per operation for rows of at
//      most kUpdShortRow entries, else a lane group per operation whose ballot names the first hit;
//   2. VALUES ONLY (every operation lands on an existing entry -- the re-assembly of a fixed pattern): a stable radix sort of the
//      operations by target (rocPRIM; the value and the op ride as payload), then one thread per run of equal targets folds it
//      in stream order from the stored value and writes the value back in place.  Structure and everything derived from it stay;
//   3. GENERAL (some operation creates an entry; SMH_APPLY_FAST=0 sends every stream here): the operations are split stably into
//      present and absent ones; the present ones are sorted by target as in 2., the absent ones by (row, column) -- a run is one
//      new entry, its head the first appearance.  The heads, sorted by (row, first appearance), give the per-row counts; the
//      device scan turns them into offsets (and decides the capacity error before the result arrays are allocated); m's
//      entries move behind their row's new ones, new entries are written reversed, and every run is folded by one thread.
// The batched get is step 1 with the stored value (or +0) as its output.
#include <rocprim/device/device_radix_sort.hpp>

#include <cstdlib>

#include "arg_stage.hpp"
#include "crs_forms.hpp"

namespace smh {

constexpr uint32_t kUpdShortRow = 64;      // longest row of m the one-thread-per-operation lookup takes
constexpr uint32_t kAbsent = 0xFFFFFFFFu;  // lookup: no entry of the row has the column

struct UpdInfo {
    uint32_t n_absent;     // operations without a target in m
    uint32_t max_row;      // largest row of any operation
    uint32_t max_new_col;  // largest column of an absent operation (valid when n_absent > 0)
    uint32_t pad;
};

__device__ __forceinline__ uint32_t upd_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, kWave);
    return v;
}

template <typename T> __device__ __forceinline__ T upd_add(T a, T b) {  // one rounding, never contracted
    if constexpr (sizeof(T) == 4) return __fadd_rn(a, b);
    else return __dadd_rn(a, b);
}

// ---- 1. lookup -------------------------------------------------------------------------------------------------------------
// G lanes per query (a power of two dividing the wavefront); the group walks the row G entries at a time and stops at the first
// chunk holding a hit, whose lowest hit lane is the first match.  VALUES: val_out[q] = stored value or +0 (get); otherwise
// idx_out[q] = entry index or kAbsent, and the info words (apply).
template <int G, typename T, bool VALUES>
__global__ void __launch_bounds__(kBlock)
k_upd_lookup(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val, uint64_t n_rows,
             const uint32_t *__restrict__ q_row, const uint32_t *__restrict__ q_col, uint64_t n, uint32_t *__restrict__ idx_out,
             T *__restrict__ val_out, UpdInfo *info) {
    const uint32_t lane = threadIdx.x & (G - 1);
    const uint32_t wbase = (threadIdx.x & (kWave - 1)) & ~(uint32_t)(G - 1);
    const uint64_t gmask = G == 64 ? ~0ull : ((1ull << G) - 1);
    const uint64_t stride = (uint64_t)gridDim.x * (blockDim.x / G);
    uint32_t n_absent = 0, max_row = 0, max_new_col = 0;
    for (uint64_t q = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G; q < n; q += stride) {
        const uint32_t i = q_row[q], c = q_col[q];
        uint32_t found = kAbsent;
        if (i < n_rows) {
            const uint32_t a0 = off[i], a1 = off[i + 1];
            for (uint32_t base = a0; base < a1; base += G) {
                const uint32_t p = base + lane;
                const bool hit = p < a1 && col[p] == c;
                if constexpr (G == 1) {
                    if (hit) { found = p; break; }
                } else {
                    const uint64_t m = ((uint64_t)__ballot(hit) >> wbase) & gmask;  // the same in every lane of the group
                    if (m) { found = base + (uint32_t)__builtin_ctzll(m); break; }
                }
            }
        }
        if (lane == 0) {
            if constexpr (VALUES) {
                val_out[q] = found == kAbsent ? T(0) : val[found];
            } else {
                idx_out[q] = found;
                max_row = i > max_row ? i : max_row;
                if (found == kAbsent) {
                    ++n_absent;
                    max_new_col = c > max_new_col ? c : max_new_col;
                }
            }
        }
    }
    if constexpr (!VALUES) {
        n_absent = upd_wave_sum(n_absent);
        max_row = wave_max_u32(max_row);
        max_new_col = wave_max_u32(max_new_col);
        if ((threadIdx.x & (kWave - 1)) == 0) {
            if (n_absent) atomicAdd(&info->n_absent, n_absent);
            atomicMax(&info->max_row, max_row);
            atomicMax(&info->max_new_col, max_new_col);
        }
    }
}

template <typename T, bool VALUES>
static int launch_lookup(uint32_t max_row_len, const uint32_t *off, const uint32_t *col, const T *val, uint64_t n_rows, const uint32_t *q_row,
                         const uint32_t *q_col, uint64_t n, uint32_t *idx_out, T *val_out, UpdInfo *info, hipStream_t s) {
    // lane groups sized from the longest row (as K1 sizes its sub-wave groups): one thread per query on short rows
    const int g = max_row_len <= kUpdShortRow ? 1 : max_row_len <= 512 ? 8 : 32;
    const unsigned grid = grid_for(n * (uint64_t)g, kBuildGrid);
    if (g == 1)
        hipLaunchKernelGGL((k_upd_lookup<1, T, VALUES>), dim3(grid), dim3(kBlock), 0, s, off, col, val, n_rows, q_row, q_col, n, idx_out, val_out, info);
    else if (g == 8)
        hipLaunchKernelGGL((k_upd_lookup<8, T, VALUES>), dim3(grid), dim3(kBlock), 0, s, off, col, val, n_rows, q_row, q_col, n, idx_out, val_out, info);
    else
        hipLaunchKernelGGL((k_upd_lookup<32, T, VALUES>), dim3(grid), dim3(kBlock), 0, s, off, col, val, n_rows, q_row, q_col, n, idx_out, val_out, info);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// ---- 2. / 3. folds and structure -------------------------------------------------------------------------------------------
// an operation as the payload of the sort by target: its value and whether it is a `set` (8 bytes f32, 16 bytes f64), so that
// the fold reads the sorted runs in order instead of gathering by stream position
template <typename T> struct UpdOp {
    T v;
    uint32_t set;
};

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_upd_payload(const T *__restrict__ vals, const uint8_t *__restrict__ ops, uint64_t n, UpdOp<T> *__restrict__ pay) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        UpdOp<T> o;
        o.v = vals[k];
        o.set = ops && ops[k] ? 1u : 0u;
        pay[k] = o;
    }
}

// one thread per run of equal targets (key sorted stably: the run is in stream order) folds it from src_val[t] and writes
// dst_val[newpos ? newpos[t] : t].  src_val may be dst_val (in place: each run reads and writes its own entry only).  A run is
// folded serially: a stream piling n operations onto one entry costs one thread n steps.
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_upd_fold(const uint32_t *__restrict__ key, const UpdOp<T> *__restrict__ pay, uint64_t n, const T *src_val, T *dst_val,
           const uint32_t *__restrict__ newpos) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t t = key[q];
        if (q > 0 && key[q - 1] == t) continue;  // folded by its run's head
        T acc = src_val[t];
        for (uint64_t q2 = q; q2 < n && key[q2] == t; ++q2) {
            const UpdOp<T> o = pay[q2];
            acc = o.set ? o.v : upd_add(acc, o.v);
        }
        dst_val[newpos ? newpos[t] : t] = acc;
    }
}

// flag[k] = 1 for an operation without a target (the caller scans the flags: pos = absent operations before k)
__global__ void __launch_bounds__(kBlock)
k_upd_absent_flags(const uint32_t *__restrict__ tgt, uint64_t n, uint32_t *__restrict__ flag) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x)
        flag[k] = tgt[k] == kAbsent ? 1u : 0u;
}

// stable split: present operations -> (target, value and op), absent ones -> ((row << cbits) | column, k)
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_upd_split(const uint32_t *__restrict__ tgt, const uint32_t *__restrict__ rows, const uint32_t *__restrict__ cols, const T *__restrict__ vals,
            const uint8_t *__restrict__ ops, uint64_t n, const uint32_t *__restrict__ pos, unsigned cbits, uint32_t *__restrict__ pkey,
            UpdOp<T> *__restrict__ ppay, uint64_t *__restrict__ akey, uint32_t *__restrict__ asrc) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t a = pos[k];
        if (pos[k + 1] != a) {
            akey[a] = ((uint64_t)rows[k] << cbits) | cols[k];
            asrc[a] = (uint32_t)k;
        } else {
            const uint64_t p = k - a;
            pkey[p] = tgt[k];
            UpdOp<T> o;
            o.v = vals[k];
            o.set = ops && ops[k] ? 1u : 0u;
            ppay[p] = o;
        }
    }
}

// flag[q] = 1 at the head of a run of equal (row, column) among the sorted absent operations: one new entry each
__global__ void __launch_bounds__(kBlock)
k_upd_head_flags(const uint64_t *__restrict__ akey, uint64_t n, uint32_t *__restrict__ flag) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (uint64_t)gridDim.x * blockDim.x)
        flag[q] = (q == 0 || akey[q - 1] != akey[q]) ? 1u : 0u;
}

// new entry h (= hpos[q] of its head q) -> key (row << kbits) | first stream position, payload q
__global__ void __launch_bounds__(kBlock)
k_upd_heads(const uint64_t *__restrict__ akey, const uint32_t *__restrict__ asrc, uint64_t n, const uint32_t *__restrict__ hpos, unsigned cbits,
            unsigned kbits, uint64_t *__restrict__ hkey, uint32_t *__restrict__ hsrc) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t h = hpos[q];
        if (hpos[q + 1] == h) continue;
        hkey[h] = ((akey[q] >> cbits) << kbits) | asrc[q];  // stable sort: the head holds the smallest stream position
        hsrc[h] = (uint32_t)q;
    }
}

// cnt[row] = new entries of the row (the heads sorted by (row, first appearance): a row's new entries are contiguous)
__global__ void __launch_bounds__(kBlock)
k_upd_count_rows(const uint64_t *__restrict__ hkey, uint64_t n_new, unsigned kbits, uint32_t *__restrict__ cnt) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_new; p += (uint64_t)gridDim.x * blockDim.x)
        atomicAdd(&cnt[hkey[p] >> kbits], 1u);  // integer counts: exact whatever the order
}

// r_off[i] = m's offset + new entries before row i, i <= n_rows (rows past m's end start at m's nnz)
__global__ void __launch_bounds__(kBlock)
k_upd_offsets(const uint32_t *__restrict__ m_off, uint64_t m_rows, const uint32_t *__restrict__ nb, uint64_t n_rows, uint32_t *__restrict__ r_off) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_rows; i += (uint64_t)gridDim.x * blockDim.x)
        r_off[i] = m_off[i < m_rows ? i : m_rows] + nb[i];
}

// m's entries behind their row's new ones; rows_newpos[p] (the row of entry p on entry) becomes p's place in the result
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_upd_move_old(const uint32_t *__restrict__ m_off, const uint32_t *__restrict__ m_col, const T *__restrict__ m_val, uint64_t nnz,
               const uint32_t *__restrict__ nb, const uint32_t *__restrict__ r_off, uint32_t *__restrict__ rows_newpos, uint32_t *__restrict__ r_col,
               T *__restrict__ r_val) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = rows_newpos[p];
        const uint32_t dst = r_off[i] + (nb[i + 1] - nb[i]) + ((uint32_t)p - m_off[i]);
        r_col[dst] = m_col[p];
        r_val[dst] = m_val[p];
        rows_newpos[p] = dst;
    }
}

// new entry p (row-major, by first appearance inside the row): written reversed (push prepends), its run folded from +0
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_upd_emit_new(const uint64_t *__restrict__ hkey, const uint32_t *__restrict__ hsrc, uint64_t n_new, unsigned kbits, const uint64_t *__restrict__ akey,
               const uint32_t *__restrict__ asrc, uint64_t n_absent, uint64_t cmask, const T *__restrict__ vals, const uint8_t *__restrict__ ops,
               const uint32_t *__restrict__ nb, const uint32_t *__restrict__ r_off, uint32_t *__restrict__ r_col, T *__restrict__ r_val) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_new; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)(hkey[p] >> kbits);
        const uint32_t n_row = nb[i + 1] - nb[i];
        const uint32_t rank = (uint32_t)p - nb[i];
        const uint32_t dst = r_off[i] + n_row - 1 - rank;
        const uint64_t q = hsrc[p], key = akey[q];
        T acc = T(0);
        for (uint64_t q2 = q; q2 < n_absent && akey[q2] == key; ++q2) {
            const uint32_t k = asrc[q2];
            const T v = vals[k];
            acc = (ops && ops[k]) ? v : upd_add(acc, v);
        }
        r_col[dst] = (uint32_t)(key & cmask);
        r_val[dst] = acc;
    }
}

// ---- driver ----------------------------------------------------------------------------------------------------------------
// stable sort of (target, operation) pairs by target, bits [0, bits)
template <typename P>
static int sort_by_target(uint32_t *key_in, uint32_t *key_out, P *src_in, P *src_out, uint64_t n, unsigned bits, hipStream_t s) {
    if (n == 0) return SMH_OK;
    SMH_ROCPRIM(s, rocprim::radix_sort_pairs(tmp, bytes, key_in, key_out, src_in, src_out, (size_t)n, 0u, bits, s));
    return SMH_OK;
}

template <typename T>
static int get_many_t(const UpdMatrix &m, uint64_t n, const uint32_t *rows, const uint32_t *cols, T *out, hipStream_t s) {
    return launch_lookup<T, true>(m.max_row_len, m.off, m.col, (const T *)m.val, m.n_rows, rows, cols, n, nullptr, out, nullptr, s);
}

int crs_get_many(int dtype, const UpdMatrix &m, size_t n, const uint32_t *rows, const uint32_t *cols, void *values_out, hipStream_t s) {
    if (n == 0) return SMH_OK;
    if (dtype == SMH_F64) SMH_TRY(get_many_t<double>(m, n, rows, cols, (double *)values_out, s));
    else SMH_TRY(get_many_t<float>(m, n, rows, cols, (float *)values_out, s));
    SMH_HIP(hipStreamSynchronize(s));
    return SMH_OK;
}

template <typename T>
static int apply_t(const UpdMatrix &m, uint64_t n, const uint32_t *rows, const uint32_t *cols, const T *vals, const uint8_t *ops, bool force_general,
                   UpdResult *res, hipStream_t s) {
    Scratch scr;
    UpdInfo *d_info = nullptr, h_info;
    uint32_t *tgt = nullptr;
    SMH_TRY(scr.alloc(&d_info, 1));
    SMH_TRY(scr.alloc(&tgt, n));
    SMH_HIP(hipMemsetAsync(d_info, 0, sizeof(UpdInfo), s));
    SMH_TRY((launch_lookup<T, false>(m.max_row_len, m.off, m.col, (const T *)m.val, m.n_rows, rows, cols, n, tgt, nullptr, d_info, s)));
    SMH_HIP(hipMemcpyAsync(&h_info, d_info, sizeof h_info, hipMemcpyDeviceToHost, s));
    SMH_HIP(hipStreamSynchronize(s));
    const uint64_t n_rows = (uint64_t)h_info.max_row + 1 > m.n_rows ? (uint64_t)h_info.max_row + 1 : m.n_rows;
    if (n_rows >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "n_rows does not fit the u32 index type");
    const unsigned tbits = bits_for(m.nnz);
    if (h_info.n_absent == 0 && !force_general) {
        // 2. values only: sort by target, fold in place
        res->route = 1;
        res->values_only = true;
        uint32_t *key = nullptr;
        UpdOp<T> *src_in = nullptr, *src = nullptr;
        SMH_TRY(scr.alloc(&key, n));
        SMH_TRY(scr.alloc(&src_in, n));
        SMH_TRY(scr.alloc(&src, n));
        hipLaunchKernelGGL((k_upd_payload<T>), dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, vals, ops, n, src_in);
        SMH_HIP(hipGetLastError());
        SMH_TRY(sort_by_target(tgt, key, src_in, src, n, tbits, s));
        hipLaunchKernelGGL((k_upd_fold<T>), dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, key, (const UpdOp<T> *)src, n, (const T *)m.val, (T *)m.val,
                           (const uint32_t *)nullptr);
        SMH_HIP(hipGetLastError());
        SMH_HIP(hipStreamSynchronize(s));
        return SMH_OK;
    }
    // 3. general
    res->route = 0;
    const uint64_t n_absent = h_info.n_absent, n_present = n - n_absent;
    uint32_t *pos = nullptr, *pkey_in = nullptr, *pkey = nullptr, *asrc_in = nullptr, *asrc = nullptr;
    UpdOp<T> *psrc_in = nullptr, *psrc = nullptr;
    uint64_t *akey_in = nullptr, *akey = nullptr;
    SMH_TRY(scr.alloc(&pos, n + 1));
    hipLaunchKernelGGL(k_upd_absent_flags, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, tgt, n, pos);
    SMH_HIP(hipGetLastError());
    SMH_HIP(hipMemsetAsync(pos + n, 0, sizeof(uint32_t), s));
    uint64_t total = 0;
    SMH_TRY(device_exclusive_scan_u32(pos, n + 1, s, &total));
    SMH_TRY(scr.alloc(&pkey_in, n_present));
    SMH_TRY(scr.alloc(&psrc_in, n_present));
    SMH_TRY(scr.alloc(&pkey, n_present));
    SMH_TRY(scr.alloc(&psrc, n_present));
    SMH_TRY(scr.alloc(&akey_in, n_absent));
    SMH_TRY(scr.alloc(&asrc_in, n_absent));
    SMH_TRY(scr.alloc(&akey, n_absent));
    SMH_TRY(scr.alloc(&asrc, n_absent));
    const unsigned cbits = bits_for(h_info.max_new_col), rbits = bits_for(h_info.max_row), kbits = bits_for(n);
    hipLaunchKernelGGL((k_upd_split<T>), dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, tgt, rows, cols, vals, ops, n, pos, cbits, pkey_in, psrc_in, akey_in,
                       asrc_in);
    SMH_HIP(hipGetLastError());
    SMH_TRY(sort_by_target(pkey_in, pkey, psrc_in, psrc, n_present, tbits, s));
    if (n_absent)
        SMH_ROCPRIM(s, rocprim::radix_sort_pairs(tmp, bytes, akey_in, akey, asrc_in, asrc, (size_t)n_absent, 0u, rbits + cbits, s));
    // new entries: heads of the (row, column) runs, sorted by (row, first appearance)
    uint32_t *hpos = nullptr, *hsrc_in = nullptr, *hsrc = nullptr, *nb = nullptr;
    uint64_t *hkey_in = nullptr, *hkey = nullptr, n_new = 0;
    SMH_TRY(scr.alloc(&hpos, n_absent + 1));
    SMH_TRY(scr.alloc(&nb, n_rows + 1));
    SMH_HIP(hipMemsetAsync(nb, 0, (n_rows + 1) * sizeof(uint32_t), s));
    if (n_absent) {
        hipLaunchKernelGGL(k_upd_head_flags, dim3(grid_for(n_absent, kBuildGrid)), dim3(kBlock), 0, s, akey, n_absent, hpos);
        SMH_HIP(hipGetLastError());
        SMH_HIP(hipMemsetAsync(hpos + n_absent, 0, sizeof(uint32_t), s));
        SMH_TRY(device_exclusive_scan_u32(hpos, n_absent + 1, s, &n_new));
        SMH_TRY(scr.alloc(&hkey_in, n_new));
        SMH_TRY(scr.alloc(&hkey, n_new));
        SMH_TRY(scr.alloc(&hsrc_in, n_new));
        SMH_TRY(scr.alloc(&hsrc, n_new));
        hipLaunchKernelGGL(k_upd_heads, dim3(grid_for(n_absent, kBuildGrid)), dim3(kBlock), 0, s, akey, asrc, n_absent, hpos, cbits, kbits, hkey_in, hsrc_in);
        SMH_HIP(hipGetLastError());
        SMH_ROCPRIM(s, rocprim::radix_sort_pairs(tmp, bytes, hkey_in, hkey, hsrc_in, hsrc, (size_t)n_new, 0u, rbits + kbits, s));
        hipLaunchKernelGGL(k_upd_count_rows, dim3(grid_for(n_new, kBuildGrid)), dim3(kBlock), 0, s, hkey, n_new, kbits, nb);
        SMH_HIP(hipGetLastError());
    }
    uint64_t n_new2 = 0;
    SMH_TRY(device_exclusive_scan_u32(nb, n_rows + 1, s, &n_new2));
    if (n_new2 != n_new) return fail(SMH_ERR_HIP, "apply: new-entry counts disagree (%llu vs %llu)", (unsigned long long)n_new2, (unsigned long long)n_new);
    // capacity: entries plus orphans below u32::MAX (sparsemat_crs.rs:82-84), decided before the result is allocated or written
    const uint64_t nnz = (uint64_t)m.nnz + n_new;
    if (nnz + m.orphans >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    res->n_rows = n_rows;
    const uint64_t new_cols = n_new ? (uint64_t)h_info.max_new_col + 1 : 0;
    res->n_cols = m.n_cols > new_cols ? m.n_cols : new_cols;
    res->nnz = nnz;
    uint32_t *rows_newpos = nullptr;
    SMH_TRY(scr.alloc(&rows_newpos, m.nnz));
    SMH_TRY(expand_rows(m.off, m.n_rows, rows_newpos, s));
    SMH_TRY(res->arrays.alloc(n_rows, nnz, sizeof(T)));  // (freed with res unless the caller takes them)
    uint32_t *r_off = res->arrays.off, *r_col = res->arrays.col;
    T *r_val = (T *)res->arrays.val;
    hipLaunchKernelGGL(k_upd_offsets, dim3(grid_for(n_rows + 1, kBuildGrid)), dim3(kBlock), 0, s, m.off, (uint64_t)m.n_rows, nb, n_rows, r_off);
    SMH_HIP(hipGetLastError());
    if (m.nnz) {
        hipLaunchKernelGGL((k_upd_move_old<T>), dim3(grid_for(m.nnz, kBuildGrid)), dim3(kBlock), 0, s, m.off, m.col, (const T *)m.val, (uint64_t)m.nnz, nb, r_off,
                           rows_newpos, r_col, r_val);
        SMH_HIP(hipGetLastError());
    }
    if (n_new) {
        hipLaunchKernelGGL((k_upd_emit_new<T>), dim3(grid_for(n_new, kBuildGrid)), dim3(kBlock), 0, s, hkey, hsrc, n_new, kbits, akey, asrc, n_absent,
                           (cbits >= 64 ? ~0ull : ((1ull << cbits) - 1)), vals, ops, nb, r_off, r_col, r_val);
        SMH_HIP(hipGetLastError());
    }
    if (n_present) {
        hipLaunchKernelGGL((k_upd_fold<T>), dim3(grid_for(n_present, kBuildGrid)), dim3(kBlock), 0, s, pkey, (const UpdOp<T> *)psrc, n_present, (const T *)m.val, r_val,
                           (const uint32_t *)rows_newpos);
        SMH_HIP(hipGetLastError());
    }
    SMH_HIP(hipStreamSynchronize(s));
    return SMH_OK;
}

// stream positions 0..n-1: the payload of the plan's sort by target
__global__ void __launch_bounds__(kBlock) k_upd_iota(uint32_t *__restrict__ out, uint64_t n) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) out[k] = (uint32_t)k;
}

// steps 1. and 2. without the values, for an update plan (matplan.hip): lookup, then the stable sort by target with the stream
// position as payload
int crs_plan_targets(const UpdMatrix &m, size_t n, const uint32_t *rows, const uint32_t *cols, uint32_t *key_out, uint32_t *src_out,
                     uint64_t *n_absent_out, hipStream_t s) {
    Scratch scr;
    UpdInfo *d_info = nullptr, h_info;
    uint32_t *tgt = nullptr, *src_in = nullptr;
    SMH_TRY(scr.alloc(&d_info, 1));
    SMH_TRY(scr.alloc(&tgt, n));
    SMH_HIP(hipMemsetAsync(d_info, 0, sizeof(UpdInfo), s));
    SMH_TRY((launch_lookup<float, false>(m.max_row_len, m.off, m.col, (const float *)nullptr, m.n_rows, rows, cols, n, tgt, nullptr, d_info, s)));
    SMH_HIP(hipMemcpyAsync(&h_info, d_info, sizeof h_info, hipMemcpyDeviceToHost, s));
    SMH_HIP(hipStreamSynchronize(s));
    *n_absent_out = h_info.n_absent;
    if (h_info.n_absent) return SMH_OK;
    SMH_TRY(scr.alloc(&src_in, n));
    hipLaunchKernelGGL(k_upd_iota, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, src_in, (uint64_t)n);
    SMH_HIP(hipGetLastError());
    return sort_by_target(tgt, key_out, src_in, src_out, n, bits_for(m.nnz), s);
}

int crs_apply(int dtype, const UpdMatrix &m, size_t n, const uint32_t *rows, const uint32_t *cols, const void *vals, const uint8_t *ops,
              bool force_general, UpdResult *res, hipStream_t s) {
    *res = UpdResult();
    if (dtype == SMH_F64) return apply_t<double>(m, n, rows, cols, (const double *)vals, ops, force_general, res, s);
    return apply_t<float>(m, n, rows, cols, (const float *)vals, ops, force_general, res, s);
}

// SparseMatrix::eye (sparsematrix.rs:91-98) for dim >= 2: offsets 0..dim, columns 0..dim-1, ones
template <typename T>
__global__ void __launch_bounds__(kBlock) k_upd_eye(uint32_t *__restrict__ off, uint32_t *__restrict__ col, T *__restrict__ val, uint64_t dim) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= dim; i += (uint64_t)gridDim.x * blockDim.x) {
        off[i] = (uint32_t)i;
        if (i < dim) {
            col[i] = (uint32_t)i;
            val[i] = T(1);
        }
    }
}

int build_eye(int dtype, size_t dim, uint32_t *off, uint32_t *col, void *val, hipStream_t s) {
    if (dtype == SMH_F64) hipLaunchKernelGGL((k_upd_eye<double>), dim3(grid_for(dim + 1, kBuildGrid)), dim3(kBlock), 0, s, off, col, (double *)val, (uint64_t)dim);
    else hipLaunchKernelGGL((k_upd_eye<float>), dim3(grid_for(dim + 1, kBuildGrid)), dim3(kBlock), 0, s, off, col, (float *)val, (uint64_t)dim);
    SMH_HIP(hipGetLastError());
    SMH_HIP(hipStreamSynchronize(s));
    return SMH_OK;
}

// ---- the entry points: SparseMatrix::get / set / add_to / eye (sparsematrix.rs:91-98, 224-233; sparsemat_crs.rs:54-92, 136-150) --
UpdMatrix upd_view(const smh_crs *m) {
    UpdMatrix u;
    u.off = m->d_off; u.col = m->d_col; u.val = m->d_val;
    u.n_rows = m->n_rows; u.n_cols = m->n_cols; u.nnz = m->nnz; u.orphans = m->orphans;
    u.max_row_len = m->max_row_len;
    return u;
}

static int get_many_common(const smh_crs *m, size_t n, const uint32_t *rows, const uint32_t *cols, void *values_out, bool on_device) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (n && (!rows || !cols || !values_out)) return fail(SMH_ERR_INVALID, "NULL query array");
    if (n == 0) return SMH_OK;
    const size_t vs = dtype_size(m->dtype);
    ArgStage st(on_device, m->device);
    if (m->n_rows == 0) {  // find_index needs i < n_rows (sparsemat_crs.rs:54-67): every answer is zero
        // known difference, kept: the query arrays are checked and waited for, never staged
        SMH_TRY(st.check(rows, "rows"));
        SMH_TRY(st.check(cols, "cols"));
        SMH_TRY(st.check(values_out, "values_out"));
        SMH_TRY(st.callers_writes_first());
        SMH_HIP(hipStreamSynchronize(m->stream));
        if (on_device) SMH_HIP(hipMemset(values_out, 0, n * vs));
        else memset(values_out, 0, n * vs);
        return SMH_OK;
    }
    const void *d_rows = nullptr, *d_cols = nullptr;
    void *d_out = nullptr;
    SMH_TRY(st.in(rows, n * sizeof(uint32_t), "rows", &d_rows));
    SMH_TRY(st.in(cols, n * sizeof(uint32_t), "cols", &d_cols));
    SMH_TRY(st.out(values_out, n * vs, "values_out", &d_out));
    SMH_TRY(st.callers_writes_first());
    SMH_HIP(hipStreamSynchronize(m->stream));
    SMH_TRY(crs_get_many(m->dtype, upd_view(m), n, (const uint32_t *)d_rows, (const uint32_t *)d_cols, d_out, m->stream));
    return st.finish();
}

static thread_local int g_apply_route = 1;

static int apply_common(smh_crs *m, size_t n, const uint32_t *rows, const uint32_t *cols, const void *values, const uint8_t *ops, bool on_device) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (n && (!rows || !cols || !values)) return fail(SMH_ERR_INVALID, "NULL operation array");
    if (n >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    if (n == 0) {  // nothing applied: m untouched
        g_apply_route = 1;
        return SMH_OK;
    }
    if (m->n_rows == 0 && m->orphans && !m->has_first_op)
        return fail(SMH_ERR_INVALID, "apply: the handle has no rows but an orphaned entry whose operation it does not know");
    const size_t vs = dtype_size(m->dtype);
    ArgStage st(on_device, m->device);
    const void *d_rows = nullptr, *d_cols = nullptr, *d_vals = nullptr, *d_ops = nullptr;
    SMH_TRY(st.in(rows, n * sizeof(uint32_t), "rows", &d_rows));
    SMH_TRY(st.in(cols, n * sizeof(uint32_t), "cols", &d_cols));
    SMH_TRY(st.in(values, n * vs, "values", &d_vals));
    SMH_TRY(st.in(ops, n, "ops", &d_ops));
    SMH_TRY(st.callers_writes_first());
    SMH_HIP(hipStreamSynchronize(m->stream));
    smh_crs *fresh = nullptr;
    if (m->n_rows == 0) {
        // SparseMatCRS::new(), or the state its first push leaves (sparsemat_crs.rs:75-76): the replay of (that push ++ the stream)
        g_apply_route = 2;
        if (!m->has_first_op) {
            SMH_TRY(assemble_common((smh_dtype)m->dtype, n, (const uint32_t *)d_rows, (const uint32_t *)d_cols, d_vals, (const uint8_t *)d_ops, true,
                                    true, &fresh));
        } else {
            Scratch cat;  // that push's operation ++ the stream
            uint32_t *c_rows = nullptr, *c_cols = nullptr;
            char *c_vals = nullptr;
            uint8_t *c_ops = nullptr;
            SMH_TRY(cat.alloc(&c_rows, n + 1));
            SMH_TRY(cat.alloc(&c_cols, n + 1));
            SMH_TRY(cat.alloc(&c_vals, (n + 1) * vs));
            SMH_TRY(cat.alloc(&c_ops, n + 1));
            const uint8_t set = 1;  // the recorded value is already folded: `set` it
            SMH_HIP(hipMemcpy(c_rows, &m->first_row, sizeof(uint32_t), hipMemcpyHostToDevice));
            SMH_HIP(hipMemcpy(c_cols, &m->first_col, sizeof(uint32_t), hipMemcpyHostToDevice));
            SMH_HIP(hipMemcpy(c_vals, &m->first_val_bits, vs, hipMemcpyHostToDevice));
            SMH_HIP(hipMemcpy(c_ops, &set, 1, hipMemcpyHostToDevice));
            SMH_HIP(hipMemcpy(c_rows + 1, d_rows, n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
            SMH_HIP(hipMemcpy(c_cols + 1, d_cols, n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
            SMH_HIP(hipMemcpy(c_vals + vs, d_vals, n * vs, hipMemcpyDeviceToDevice));
            if (d_ops) SMH_HIP(hipMemcpy(c_ops + 1, d_ops, n, hipMemcpyDeviceToDevice));
            else SMH_HIP(hipMemset(c_ops + 1, 0, n));
            SMH_TRY(assemble_common((smh_dtype)m->dtype, n + 1, c_rows, c_cols, c_vals, c_ops, true, true, &fresh));
        }
        if (fresh->n_cols < m->n_cols) fresh->n_cols = m->n_cols;  // push only raises n_cols (sparsemat_crs.rs:72-74)
        fresh->knobs = m->knobs;
        replace_state(m, fresh, false);
        return SMH_OK;
    }
    const bool force_general = getenv("SMH_APPLY_FAST") && atoi(getenv("SMH_APPLY_FAST")) == 0;
    UpdResult r;
    SMH_TRY(crs_apply(m->dtype, upd_view(m), n, (const uint32_t *)d_rows, (const uint32_t *)d_cols, d_vals, (const uint8_t *)d_ops, force_general, &r,
                      m->stream));
    g_apply_route = r.route;
    if (r.values_only)  // structure unchanged: every form derived from it stays, the value-derived ones are refreshed
        return smh_crs_update_values(m, nullptr);
    SMH_TRY(wrap_arrays(m->dtype, m, r.n_rows, r.n_cols, r.nnz, r.arrays, 0, &fresh));
    fresh->orphans = m->orphans;
    replace_state(m, fresh, false);
    return SMH_OK;
}

}  // namespace smh

using namespace smh;

extern "C" {

int smh_last_apply_route(void) { return g_apply_route; }

int smh_crs_get(const smh_crs *m, size_t i, size_t j, void *value_out) {
    if (!m || !value_out) return fail(SMH_ERR_INVALID, "NULL argument");
    if (i >= m->n_rows || j > 0xFFFFFFFFull) {  // no row i, or a column no entry can have
        memset(value_out, 0, dtype_size(m->dtype));
        return SMH_OK;
    }
    const uint32_t r = (uint32_t)i, c = (uint32_t)j;
    return get_many_common(m, 1, &r, &c, value_out, false);
}
int smh_crs_get_many(const smh_crs *m, size_t n, const uint32_t *rows, const uint32_t *cols, void *values_out) {
    return get_many_common(m, n, rows, cols, values_out, false);
}
int smh_crs_get_many_dev(const smh_crs *m, size_t n, const uint32_t *rows_dev, const uint32_t *cols_dev, void *values_out_dev) {
    return get_many_common(m, n, rows_dev, cols_dev, values_out_dev, true);
}

int smh_crs_apply(smh_crs *m, size_t n_ops, const uint32_t *rows, const uint32_t *cols, const void *values, const uint8_t *ops) {
    return apply_common(m, n_ops, rows, cols, values, ops, false);
}
int smh_crs_apply_dev(smh_crs *m, size_t n_ops, const uint32_t *rows_dev, const uint32_t *cols_dev, const void *values_dev, const uint8_t *ops_dev) {
    return apply_common(m, n_ops, rows_dev, cols_dev, values_dev, ops_dev, true);
}

int smh_crs_eye(smh_dtype dtype, size_t dim, smh_crs **out) {
    if (!out) return fail(SMH_ERR_INVALID, "NULL out pointer");
    *out = nullptr;
    if (!valid_dtype(dtype)) return fail(SMH_ERR_INVALID, "dtype must be SMH_F32 or SMH_F64");
    if (dim >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    SMH_TRY(require_device());
    if (dim <= 1) {  // no rows (dim 0); the first push alone: no rows, one orphan, n_cols 1 (dim 1)
        const uint32_t zero = 0;
        const uint8_t set = 1;
        const double one64 = 1.0;
        const float one32 = 1.0f;
        return assemble_common(dtype, dim, &zero, &zero, dtype == SMH_F64 ? (const void *)&one64 : (const void *)&one32, &set, false, true, out);
    }
    CrsArrays arrays;
    SMH_TRY(arrays.alloc(dim, dim, dtype_size(dtype)));
    SMH_TRY(build_eye(dtype, dim, arrays.off, arrays.col, arrays.val, nullptr));
    return wrap_arrays(dtype, nullptr, dim, dim, dim, arrays, 0, out);
}

}  // extern "C"
