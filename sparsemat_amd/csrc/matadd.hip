// matadd.hip -- SparseMatrix::add / sub (sparsematrix.rs:123-143) of two SparseMatCRS on the device, gfx950.
//
// What it replaces.  `a.add(&b)` runs `*a.get_mut(i, j) += val` for every entry of b in storage order; get_mut is
// find_index (the FIRST match in the row, sparsemat_crs.rs:54-67) or else push, which inserts at the START of the row
// (:71-92).  On the host that is O(nnz * row length) compares plus a Vec::insert per new entry.  The result is fully
// determined by the operands (tests/add_model.py restates it):
//   * row i = the new columns of b's row i in REVERSE order of first appearance, then a's row i unchanged in order;
//   * a b entry whose column exists in a's row folds into the first occurrence; a new column folds from T::zero();
//     folds are sequential in b's storage order, one rounding per operation (acc + v, acc - v for sub);
//   * n_rows = max(a.n_rows, 1 + last row of b holding an entry), n_cols = max(a.n_cols, 1 + largest NEW column).
// Device formulation (integer structure and values bit for bit, no float atomics: the fold order is the contract):
//   1. count pass -> new entries per row, plus three integers: is b entry k landing on a entry k for every k ("same
//      pattern"), the largest new column, the last row of b holding an entry;
//   2. exclusive scan of the counts (device_exclusive_scan_u32) = where each result row starts beyond a's offsets --
//      the total decides the capacity error before anything is allocated;
//   3. emit pass: every target folds its b entries in storage order; a's entries keep their order after the new ones.
// Routes (same bits on every route; smh_last_add_route reports which one ran):
//   3 SAME PATTERN: b entry k lands on a entry k for all k (identical offsets and columns, no column repeated inside
//     a row): r[k] = a[k] +- b[k] with 16-byte loads and stores, offsets and columns copied (or left in place);
//   2 STRUCTURE UNCHANGED: every b entry lands on an existing entry (a diagonal shift of a matrix with its diagonal,
//     repeated columns in a): the emit pass writes values only;
//   1 SHORT ROWS (both operands' rows at most kAddShortRow entries): one thread per row; its compares stay in the
//     row's cache lines (stencils, FEM, graph rows);
//   0 GENERAL (any row length; SMH_ADD_FAST=0 forces it): a and b's rows merged per row and sorted stably by column
//     (rocPRIM segmented radix sort), so a's entries of a column come before b's and b's keep their storage order; one
//     thread per run of equal columns folds it.  Cost O(nnz) passes plus the sort: it does not grow as lenA * lenB.
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <cstdlib>

#include "crs_forms.hpp"

namespace smh {

constexpr uint32_t kAddShortRow = 64;  // longest row (of a or b) the one-thread-per-row passes take

// info words of the count passes
struct AddInfo {
    uint32_t not_same;    // some b entry k does not land on a entry k
    uint32_t max_new_p1;  // largest column of a new entry + 1 (0: none)
    uint32_t last_b_p1;   // last row of b holding an entry + 1 (0: none)
    uint32_t pad;
};

// row bounds of an operand with n rows, for any row index (rows past the end are empty)
__device__ __forceinline__ uint32_t off_at(const uint32_t *__restrict__ off, uint64_t n, uint64_t i) { return off[i < n ? i : n]; }

__device__ __forceinline__ void info_reduce(AddInfo *info, uint32_t not_same, uint32_t max_new_p1, uint32_t last_b_p1) {
    not_same = wave_max_u32(not_same);
    max_new_p1 = wave_max_u32(max_new_p1);
    last_b_p1 = wave_max_u32(last_b_p1);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (not_same) atomicOr(&info->not_same, 1u);
        if (max_new_p1) atomicMax(&info->max_new_p1, max_new_p1);
        if (last_b_p1) atomicMax(&info->last_b_p1, last_b_p1);
    }
}

template <typename T, bool SUB> __device__ __forceinline__ T fold(T acc, T v) { return SUB ? acc - v : acc + v; }

// ---- route 1 / 2: one thread per row --------------------------------------------------------------------------------
// cnt[i] = new entries of row i (i < n_rows_max = max(a_rows, b_rows))
__global__ void __launch_bounds__(kBlock)
k_add_count(const uint32_t *__restrict__ a_off, const uint32_t *__restrict__ a_col, uint64_t a_rows, const uint32_t *__restrict__ b_off,
            const uint32_t *__restrict__ b_col, uint64_t b_rows, uint64_t n_rows_max, uint32_t *__restrict__ cnt, AddInfo *info) {
    uint32_t not_same = 0, max_new_p1 = 0, last_b_p1 = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows_max; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t a0 = off_at(a_off, a_rows, i), a1 = off_at(a_off, a_rows, i + 1);
        const uint32_t b0 = off_at(b_off, b_rows, i), b1 = off_at(b_off, b_rows, i + 1);
        uint32_t n_new = 0;
        for (uint32_t k = b0; k < b1; ++k) {
            const uint32_t c = b_col[k];
            bool found = false;
            for (uint32_t p = a0; p < a1 && !found; ++p) {
                found = a_col[p] == c;
                if (found && p != k) not_same = 1;
            }
            if (found) continue;
            not_same = 1;
            bool seen = false;
            for (uint32_t q = b0; q < k; ++q)
                if (b_col[q] == c) { seen = true; break; }
            if (!seen) {
                ++n_new;
                max_new_p1 = c + 1 > max_new_p1 ? c + 1 : max_new_p1;
            }
        }
        cnt[i] = n_new;
        if (b1 > b0) last_b_p1 = (uint32_t)(i + 1);
    }
    info_reduce(info, not_same, max_new_p1, last_b_p1);
}

// nb = exclusive scan of cnt (n_rows_max + 1 entries).  values_only: no new entry anywhere, r_val may be a_val itself
// (each thread reads and writes only its own row's values; b's values must not alias a's then)
template <typename T, bool SUB>
__global__ void __launch_bounds__(kBlock)
k_add_emit_rows(const uint32_t *__restrict__ a_off, const uint32_t *__restrict__ a_col, const T *a_val, uint64_t a_rows,
                const uint32_t *__restrict__ b_off, const uint32_t *__restrict__ b_col, const T *__restrict__ b_val, uint64_t b_rows,
                uint64_t n_rows, const uint32_t *__restrict__ nb, uint32_t *__restrict__ r_col, T *r_val, bool values_only) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t a0 = off_at(a_off, a_rows, i), a1 = off_at(a_off, a_rows, i + 1);
        const uint32_t b0 = off_at(b_off, b_rows, i), b1 = off_at(b_off, b_rows, i + 1);
        const uint32_t n_new = nb[i + 1] - nb[i];
        const uint64_t base = (uint64_t)a0 + nb[i];
        if (!values_only && n_new) {
            uint32_t r = 0;
            for (uint32_t k = b0; k < b1; ++k) {
                const uint32_t c = b_col[k];
                bool old = false;
                for (uint32_t p = a0; p < a1 && !old; ++p) old = a_col[p] == c;
                for (uint32_t q = b0; q < k && !old; ++q) old = b_col[q] == c;
                if (old) continue;
                T acc = fold<T, SUB>(T(0), b_val[k]);
                for (uint32_t q = k + 1; q < b1; ++q)
                    if (b_col[q] == c) acc = fold<T, SUB>(acc, b_val[q]);
                const uint64_t dst = base + n_new - 1 - r++;  // push prepends: first appearance ends up last
                r_col[dst] = c;
                r_val[dst] = acc;
            }
        }
        for (uint32_t p = a0; p < a1; ++p) {
            const uint32_t c = a_col[p];
            T acc = a_val[p];
            bool first = true;
            for (uint32_t q = a0; q < p && first; ++q) first = a_col[q] != c;
            if (first)
                for (uint32_t k = b0; k < b1; ++k)
                    if (b_col[k] == c) acc = fold<T, SUB>(acc, b_val[k]);
            const uint64_t dst = values_only ? p : base + n_new + (p - a0);
            if (!values_only) r_col[dst] = c;
            r_val[dst] = acc;
        }
    }
}

// r_off[i] = a's offset + new entries before row i, i <= n_rows
__global__ void __launch_bounds__(kBlock)
k_add_offsets(const uint32_t *__restrict__ a_off, uint64_t a_rows, const uint32_t *__restrict__ nb, uint64_t n_rows, uint32_t *__restrict__ r_off) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_rows; i += (uint64_t)gridDim.x * blockDim.x)
        r_off[i] = off_at(a_off, a_rows, i) + nb[i];
}

// ---- route 3: same pattern, element-wise ------------------------------------------------------------------------------
// 16-byte vectors (f32 x 4, f64 x 2); the arrays are 16-byte aligned (library arrays and smh_crs_create_dev's rule)
template <typename T, bool SUB>
__global__ void __launch_bounds__(kBlock)
k_add_same(const T *a, const T *__restrict__ b, T *r, uint64_t n) {
    constexpr int V = 16 / sizeof(T);
    typedef T vec __attribute__((ext_vector_type(V)));
    const uint64_t n_vec = n / V;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_vec; v += stride) {
        const vec x = reinterpret_cast<const vec *>(a)[v];
        const vec y = reinterpret_cast<const vec *>(b)[v];
        vec z;
#pragma unroll
        for (int j = 0; j < V; ++j) z[j] = fold<T, SUB>(x[j], y[j]);
        reinterpret_cast<vec *>(r)[v] = z;
    }
    for (uint64_t k = n_vec * V + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) r[k] = fold<T, SUB>(a[k], b[k]);
}

// ---- route 0: merged rows sorted by column -------------------------------------------------------------------------
// m_off[i] = a_off[i] + b_off[i]: row i of the merge holds a's row then b's row
__global__ void __launch_bounds__(kBlock)
k_add_merge_offsets(const uint32_t *__restrict__ a_off, uint64_t a_rows, const uint32_t *__restrict__ b_off, uint64_t b_rows, uint64_t n_rows_max,
                    uint32_t *__restrict__ m_off) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_rows_max; i += (uint64_t)gridDim.x * blockDim.x)
        m_off[i] = off_at(a_off, a_rows, i) + off_at(b_off, b_rows, i);
}

// merged keys (column) and sources (a entry p -> p, b entry k -> nnz_a + k); rows[] = row of every entry of the operand
__global__ void __launch_bounds__(kBlock)
k_add_merge_fill(const uint32_t *__restrict__ col, const uint32_t *__restrict__ rows, uint64_t n, const uint32_t *__restrict__ other_off,
                 uint64_t other_rows, bool is_b, uint32_t nnz_a, uint32_t *__restrict__ key, uint32_t *__restrict__ src) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = rows[p];
        // a entry: after b's entries of the rows before; b entry: after a's entries up to and including its row
        const uint64_t m = p + off_at(other_off, other_rows, is_b ? (uint64_t)i + 1 : (uint64_t)i);
        key[m] = col[p];
        src[m] = is_b ? nnz_a + (uint32_t)p : (uint32_t)p;
    }
}

__device__ __forceinline__ bool run_head(const uint32_t *__restrict__ key, const uint32_t *__restrict__ m_off, const uint32_t *__restrict__ m_row,
                                         uint64_t q) {
    return q == m_off[m_row[q]] || key[q - 1] != key[q];
}

// flag[k] = 1: b entry k opens a new entry (heads of runs without an a entry)
__global__ void __launch_bounds__(kBlock)
k_add_merge_flags(const uint32_t *__restrict__ key, const uint32_t *__restrict__ src, const uint32_t *__restrict__ m_off,
                  const uint32_t *__restrict__ m_row, uint64_t n_m, uint32_t nnz_a, uint32_t *__restrict__ flag, AddInfo *info) {
    uint32_t max_new_p1 = 0, last_b_p1 = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_m; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t s = src[q];
        if (s < nnz_a) continue;
        last_b_p1 = m_row[q] + 1 > last_b_p1 ? m_row[q] + 1 : last_b_p1;
        if (run_head(key, m_off, m_row, q)) {
            flag[s - nnz_a] = 1u;
            max_new_p1 = key[q] + 1 > max_new_p1 ? key[q] + 1 : max_new_p1;
        }
    }
    info_reduce(info, 0u, max_new_p1, last_b_p1);
}

// nb[i] = fs[b_off[i]]: new entries before row i (fs = exclusive scan of the flags, nnz_b + 1 entries)
__global__ void __launch_bounds__(kBlock)
k_add_rows_from_flags(const uint32_t *__restrict__ b_off, uint64_t b_rows, const uint32_t *__restrict__ fs, uint64_t n_rows_max,
                      uint32_t *__restrict__ nb) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_rows_max; i += (uint64_t)gridDim.x * blockDim.x)
        nb[i] = fs[off_at(b_off, b_rows, i)];
}

template <typename T, bool SUB>
__global__ void __launch_bounds__(kBlock)
k_add_merge_emit(const uint32_t *__restrict__ key, const uint32_t *__restrict__ src, const uint32_t *__restrict__ m_off,
                 const uint32_t *__restrict__ m_row, uint64_t n_m, const uint32_t *__restrict__ a_off, uint64_t a_rows, const T *a_val,
                 uint32_t nnz_a, const uint32_t *__restrict__ b_off, uint64_t b_rows, const T *__restrict__ b_val, const uint32_t *__restrict__ fs,
                 const uint32_t *__restrict__ nb, uint32_t *__restrict__ r_col, T *r_val, bool values_only) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_m; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t s = src[q], i = m_row[q], c = key[q];
        const bool head = run_head(key, m_off, m_row, q);
        if (s >= nnz_a && !head) continue;  // folded by its run's head
        const uint32_t a0 = off_at(a_off, a_rows, i);
        const uint32_t n_new = nb[i + 1] - nb[i];
        const uint64_t base = (uint64_t)a0 + nb[i];
        T acc;
        uint64_t dst;
        if (s < nnz_a) {
            acc = a_val[s];
            dst = values_only ? s : base + n_new + (s - a0);
        } else {
            const uint32_t k = s - nnz_a;
            acc = fold<T, SUB>(T(0), b_val[k]);
            dst = base + n_new - 1 - (fs[k] - nb[i]);
        }
        if (head) {  // the rest of the run: a's later repeats (left alone), then b's entries in storage order
            const uint32_t end = m_off[i + 1];
            for (uint64_t q2 = q + 1; q2 < end && key[q2] == c; ++q2) {
                const uint32_t s2 = src[q2];
                if (s2 >= nnz_a) acc = fold<T, SUB>(acc, b_val[s2 - nnz_a]);
            }
        }
        if (!values_only) r_col[dst] = c;
        r_val[dst] = acc;
    }
}

// ---- driver ---------------------------------------------------------------------------------------------------------
template <typename T, bool SUB>
static int add_t(const AddOperand &a, const AddOperand &b, bool in_place, bool alias, bool force_general, AddResult *res, hipStream_t s) {
    const uint64_t n_rows_max = a.n_rows > b.n_rows ? a.n_rows : b.n_rows;
    const bool short_rows = !force_general && a.max_row_len <= kAddShortRow && b.max_row_len <= kAddShortRow;
    Scratch scr;
    AddInfo *d_info = nullptr, h_info;
    uint32_t *nb = nullptr;  // new entries before each row: n_rows_max + 1
    SMH_TRY(scr.alloc(&d_info, 1));
    SMH_TRY(scr.alloc(&nb, n_rows_max + 1));
    SMH_HIP(hipMemsetAsync(d_info, 0, sizeof(AddInfo), s));
    uint64_t n_new = 0;
    // general route state
    uint32_t *key = nullptr, *src = nullptr, *m_off = nullptr, *m_row = nullptr, *fs = nullptr;
    uint64_t n_m = 0;
    if (short_rows) {
        hipLaunchKernelGGL(k_add_count, dim3(grid_for(n_rows_max, kBuildGrid)), dim3(kBlock), 0, s, a.off, a.col, (uint64_t)a.n_rows, b.off, b.col,
                           (uint64_t)b.n_rows, n_rows_max, nb, d_info);
        SMH_HIP(hipGetLastError());
        SMH_HIP(hipMemsetAsync(nb + n_rows_max, 0, sizeof(uint32_t), s));
        SMH_TRY(device_exclusive_scan_u32(nb, n_rows_max + 1, s, &n_new));
    } else {
        n_m = (uint64_t)a.nnz + b.nnz;
        if (n_m >= 0xFFFFFFFFull) return fail(SMH_ERR_INVALID, "add / sub: the general route takes operands holding fewer than 2^32 - 1 entries together");
        uint32_t *key_in = nullptr, *src_in = nullptr, *rows_a = nullptr, *rows_b = nullptr;
        SMH_TRY(scr.alloc(&key_in, n_m));
        SMH_TRY(scr.alloc(&src_in, n_m));
        SMH_TRY(scr.alloc(&key, n_m));
        SMH_TRY(scr.alloc(&src, n_m));
        SMH_TRY(scr.alloc(&m_off, n_rows_max + 1));
        SMH_TRY(scr.alloc(&m_row, n_m));
        SMH_TRY(scr.alloc(&fs, (uint64_t)b.nnz + 1));
        hipLaunchKernelGGL(k_add_merge_offsets, dim3(grid_for(n_rows_max + 1, kBuildGrid)), dim3(kBlock), 0, s, a.off, (uint64_t)a.n_rows, b.off,
                           (uint64_t)b.n_rows, n_rows_max, m_off);
        SMH_HIP(hipGetLastError());
        // rows of the operands' entries: m_row doubles as a's, key as b's (both rewritten below)
        rows_a = m_row;
        rows_b = key;
        SMH_TRY(expand_rows(a.off, a.n_rows, rows_a, s));
        SMH_TRY(expand_rows(b.off, b.n_rows, rows_b, s));
        hipLaunchKernelGGL(k_add_merge_fill, dim3(grid_for(a.nnz, kBuildGrid)), dim3(kBlock), 0, s, a.col, rows_a, (uint64_t)a.nnz, b.off, (uint64_t)b.n_rows,
                           false, (uint32_t)a.nnz, key_in, src_in);
        SMH_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_add_merge_fill, dim3(grid_for(b.nnz, kBuildGrid)), dim3(kBlock), 0, s, b.col, rows_b, (uint64_t)b.nnz, a.off, (uint64_t)a.n_rows,
                           true, (uint32_t)a.nnz, key_in, src_in);
        SMH_HIP(hipGetLastError());
        const uint32_t max_col = a.max_col > b.max_col ? a.max_col : b.max_col;
        SMH_ROCPRIM(s, rocprim::segmented_radix_sort_pairs(tmp, bytes, key_in, key, src_in, src, (unsigned)n_m, (unsigned)n_rows_max, m_off,
                                                           m_off + 1, 0u, bits_for(max_col), s));
        SMH_TRY(expand_rows(m_off, n_rows_max, m_row, s));
        SMH_HIP(hipMemsetAsync(fs, 0, ((uint64_t)b.nnz + 1) * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_add_merge_flags, dim3(grid_for(n_m, kBuildGrid)), dim3(kBlock), 0, s, key, src, m_off, m_row, n_m, (uint32_t)a.nnz, fs, d_info);
        SMH_HIP(hipGetLastError());
        SMH_TRY(device_exclusive_scan_u32(fs, (uint64_t)b.nnz + 1, s, &n_new));
        hipLaunchKernelGGL(k_add_rows_from_flags, dim3(grid_for(n_rows_max + 1, kBuildGrid)), dim3(kBlock), 0, s, b.off, (uint64_t)b.n_rows, fs, n_rows_max, nb);
        SMH_HIP(hipGetLastError());
    }
    SMH_HIP(hipMemcpyAsync(&h_info, d_info, sizeof h_info, hipMemcpyDeviceToHost, s));
    SMH_HIP(hipStreamSynchronize(s));
    // capacity: entries plus orphans below u32::MAX (sparsemat_crs.rs:82-84), decided before anything is allocated or written
    const uint64_t nnz = (uint64_t)a.nnz + n_new;
    if (nnz + a.orphans >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    const uint64_t n_rows = a.n_rows > h_info.last_b_p1 ? a.n_rows : h_info.last_b_p1;
    res->n_rows = n_rows;
    res->n_cols = a.n_cols > h_info.max_new_p1 ? a.n_cols : h_info.max_new_p1;
    res->nnz = nnz;
    const bool same = short_rows && a.nnz == b.nnz && !h_info.not_same;
    const bool values_only = n_new == 0;
    res->route = force_general || !short_rows ? 0 : same ? 3 : values_only ? 2 : 1;
    res->values_only = in_place && values_only;
    const T *b_val = (const T *)b.val;
    if (res->values_only && alias && !same) {  // a += a folding through repeats: read b's values from a snapshot
        T *snap = nullptr;
        SMH_TRY(scr.alloc(&snap, b.nnz));
        SMH_HIP(hipMemcpyAsync(snap, b.val, (size_t)b.nnz * sizeof(T), hipMemcpyDeviceToDevice, s));
        b_val = snap;
    }
    if (!res->values_only) SMH_TRY(res->arrays.alloc(n_rows, nnz, sizeof(T)));  // (freed with res unless the caller takes them)
    uint32_t *r_off = res->arrays.off, *r_col = res->arrays.col;
    T *r_val = res->values_only ? (T *)a.val : (T *)res->arrays.val;
    if (same) {
        if (!res->values_only) {
            SMH_HIP(hipMemcpyAsync(r_off, a.off, (n_rows + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
            if (nnz) SMH_HIP(hipMemcpyAsync(r_col, a.col, nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        }
        if (nnz) {
            hipLaunchKernelGGL((k_add_same<T, SUB>), dim3(grid_for((nnz + 16 / sizeof(T) - 1) / (16 / sizeof(T)), kBuildGrid)), dim3(kBlock), 0, s,
                               (const T *)a.val, b_val, r_val, nnz);
            SMH_HIP(hipGetLastError());
        }
    } else {
        if (!res->values_only) {
            hipLaunchKernelGGL(k_add_offsets, dim3(grid_for(n_rows + 1, kBuildGrid)), dim3(kBlock), 0, s, a.off, (uint64_t)a.n_rows, nb, n_rows, r_off);
            SMH_HIP(hipGetLastError());
        }
        if (short_rows) {
            hipLaunchKernelGGL((k_add_emit_rows<T, SUB>), dim3(grid_for(n_rows, kBuildGrid)), dim3(kBlock), 0, s, a.off, a.col, (const T *)a.val,
                               (uint64_t)a.n_rows, b.off, b.col, b_val, (uint64_t)b.n_rows, n_rows, nb, r_col, r_val, res->values_only);
        } else {
            hipLaunchKernelGGL((k_add_merge_emit<T, SUB>), dim3(grid_for(n_m, kBuildGrid)), dim3(kBlock), 0, s, key, src, m_off, m_row, n_m, a.off,
                               (uint64_t)a.n_rows, (const T *)a.val, (uint32_t)a.nnz, b.off, (uint64_t)b.n_rows, b_val, fs, nb, r_col, r_val,
                               res->values_only);
        }
        SMH_HIP(hipGetLastError());
    }
    SMH_HIP(hipStreamSynchronize(s));
    return SMH_OK;
}

int add_crs(int dtype, bool subtract, const AddOperand &a, const AddOperand &b, bool in_place, bool alias, bool force_general, AddResult *res,
            hipStream_t s) {
    *res = AddResult();
    if (dtype == SMH_F64)
        return subtract ? add_t<double, true>(a, b, in_place, alias, force_general, res, s)
                        : add_t<double, false>(a, b, in_place, alias, force_general, res, s);
    return subtract ? add_t<float, true>(a, b, in_place, alias, force_general, res, s)
                    : add_t<float, false>(a, b, in_place, alias, force_general, res, s);
}

}  // namespace smh

using namespace smh;

extern "C" {

// ---- the entry points: #[derive(Clone)] (sparsemat_crs.rs:8) and SparseMatrix::add / sub (sparsematrix.rs:123-143) --------------
static thread_local int g_add_route = 2;
int smh_last_add_route(void) { return g_add_route; }

int smh_crs_clone(const smh_crs *a, smh_crs **out) {
    if (!a || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    *out = nullptr;
    SMH_HIP(hipStreamSynchronize(a->stream));
    const size_t vs = dtype_size(a->dtype);
    CrsArrays arrays;
    SMH_TRY(arrays.alloc(a->n_rows, a->nnz, vs));
    SMH_HIP(hipMemcpy(arrays.off, a->d_off, (a->n_rows + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    if (a->nnz) {
        SMH_HIP(hipMemcpy(arrays.col, a->d_col, a->nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        SMH_HIP(hipMemcpy(arrays.val, a->d_val, a->nnz * vs, hipMemcpyDeviceToDevice));
    }
    SMH_TRY(wrap_arrays(a->dtype, a, a->n_rows, a->n_cols, a->nnz, arrays, 0, out));
    (*out)->orphans = a->orphans;
    (*out)->has_first_op = a->has_first_op;
    (*out)->first_row = a->first_row;
    (*out)->first_col = a->first_col;
    (*out)->first_val_bits = a->first_val_bits;
    return SMH_OK;
}

// a_mut != NULL: a += b in place (a_mut == a); else *out = a.clone() + b
static int add_common(smh_crs *a_mut, const smh_crs *a, const smh_crs *b, bool subtract, smh_crs **out) {
    if (!a || !b || (!a_mut && !out)) return fail(SMH_ERR_INVALID, "NULL argument");
    if (out) *out = nullptr;
    if (a->dtype != b->dtype) return fail(SMH_ERR_INVALID, "operands differ in value type");
    if (a->device != b->device) return fail(SMH_ERR_INVALID, "operands live on different devices");
    if (a->n_rows == 0 && a->orphans)
        return fail(SMH_ERR_INVALID, "add / sub: the left operand has no rows but an orphaned entry -- the reference's hidden offset_rows "
                                     "length decides whether it comes back to life, and the handle does not keep it");
    SMH_HIP(hipStreamSynchronize(b->stream));  // b's reads come after whatever b's stream still has to do
    SMH_HIP(hipStreamSynchronize(a->stream));
    g_add_route = 2;
    if (b->nnz == 0) {  // nothing visited: a unchanged (b's orphan is not reached by any row)
        if (a_mut) return SMH_OK;
        return smh_crs_clone(a, out);
    }
    smh_crs *fresh = nullptr;
    if (a->n_rows == 0) {
        // SparseMatCRS::new() (no offset_rows): the replay of b's entries as add_to operations, first-push quirk included
        g_add_route = 0;
        const size_t vs = dtype_size(a->dtype);
        Scratch scr;
        uint32_t *rows = nullptr;
        char *neg = nullptr;
        SMH_TRY(scr.alloc(&rows, b->nnz));
        SMH_TRY(expand_rows(b->d_off, b->n_rows, rows, nullptr));
        if (subtract) {  // 0 - v == 0 + (-v) in IEEE 754, signed zeros included
            SMH_TRY(scr.alloc(&neg, (b->nnz + 4) * vs));
            SMH_HIP(hipMemcpy(neg, b->d_val, b->nnz * vs, hipMemcpyDeviceToDevice));
            SMH_TRY(launch_scale_values(a->dtype, neg, b->nnz, -1.0, nullptr));
        }
        SMH_HIP(hipStreamSynchronize(nullptr));
        SMH_TRY(assemble_common((smh_dtype)a->dtype, b->nnz, rows, b->d_col, subtract ? (const void *)neg : b->d_val, nullptr, true, true, &fresh));
        if (fresh->n_cols < a->n_cols) fresh->n_cols = a->n_cols;  // push only raises n_cols (sparsemat_crs.rs:72-74)
        fresh->knobs = a->knobs;
        if (a_mut) replace_state(a_mut, fresh, false);
        else *out = fresh;
        return SMH_OK;
    }
    AddOperand oa, ob;
    oa.off = a->d_off; oa.col = a->d_col; oa.val = a->d_val;
    oa.n_rows = a->n_rows; oa.n_cols = a->n_cols; oa.nnz = a->nnz; oa.orphans = a->orphans;
    oa.max_row_len = a->max_row_len; oa.max_col = a->max_col;
    ob.off = b->d_off; ob.col = b->d_col; ob.val = b->d_val;
    ob.n_rows = b->n_rows; ob.n_cols = b->n_cols; ob.nnz = b->nnz; ob.orphans = b->orphans;
    ob.max_row_len = b->max_row_len; ob.max_col = b->max_col;
    const bool force_general = getenv("SMH_ADD_FAST") && atoi(getenv("SMH_ADD_FAST")) == 0;
    AddResult r;
    SMH_TRY(add_crs(a->dtype, subtract, oa, ob, a_mut != nullptr, a == b, force_general, &r, a->stream));
    g_add_route = r.route;
    if (r.values_only) {  // (borrowed by the fresh handle until it has been built: a failure must not free a's arrays)
        SMH_TRY(wrap_arrays(a->dtype, a, a->n_rows, a->n_cols, a->nnz, a->d_off, a->d_col, a->d_val, false, 0, &fresh));
        fresh->owns = a->owns;
    } else
        SMH_TRY(wrap_arrays(a->dtype, a, r.n_rows, r.n_cols, r.nnz, r.arrays, 0, &fresh));
    fresh->orphans = a->orphans;
    if (a_mut) replace_state(a_mut, fresh, r.values_only);
    else *out = fresh;
    return SMH_OK;
}

int smh_crs_add(const smh_crs *a, const smh_crs *b, smh_crs **out) { return add_common(nullptr, a, b, false, out); }
int smh_crs_sub(const smh_crs *a, const smh_crs *b, smh_crs **out) { return add_common(nullptr, a, b, true, out); }
int smh_crs_add_assign(smh_crs *a, const smh_crs *b) { return add_common(a, a, b, false, nullptr); }
int smh_crs_sub_assign(smh_crs *a, const smh_crs *b) { return add_common(a, a, b, true, nullptr); }

}  // extern "C"
