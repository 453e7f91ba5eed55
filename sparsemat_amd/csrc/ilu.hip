// ilu.hip -- the incomplete LU factorization without fill, ILU(0), of a CRS handle on its own pattern, gfx950.  An EXTENSION: the
// reference has none.
//
// F = ilu0(A) is a clone of A whose values are the unit-lower factor L on the stored (i, c) with c < i and U on those with c >= i.
// The contract (w starts as A's values; every operation rounded once, nothing fused; rows strictly ascending, every (i, i) stored):
//   for i = 0 .. n-1:
//     for kk = off[i] .. off[i+1]-1 in storage order, k = col[kk], while k < i:
//         w[kk] = w[kk] / w[diagpos[k]]
//         for jj = diagpos[k]+1 .. off[k+1]-1  (j = col[jj] > k):
//             if row i stores column j at position t:  w[t] = w[t] - w[kk] * w[jj]
//
// Schedule: row i depends on exactly the rows k < i it stores -- the LOWER TriSchedule of the pattern (trisolve.hip), whose rows,
// level_ptr, diagpos and launch plan are used as they are: a level of more than kTriSmallRows rows is one launch on a grid, a run of
// smaller levels one single-workgroup launch with a barrier between levels.  No kernel waits for a value another workgroup writes.
//
// Kernel: a group of L lanes per row (L as the solve's, tri_lanes).  The k loop of a row is sequential; the jj loop runs over the
// lanes, each of which finds t by binary search in row i's ascending columns.  Distinct jj hit distinct t and every w[t] takes its
// updates in ascending k, so each L gives the contract's bits.  A row of at most kIluSlice * L entries is factored in the group's
// slice of the LDS (columns and values) and written back once; a longer one is factored where it lies, through workgroup-scope
// atomic loads and stores with a workgroup fence after every k step (the group is part of one wavefront, so it arrives together).
#include "crs_forms.hpp"
#include "solver_tree.hpp"

#include <cstdint>

using namespace smh;

namespace {

// LDS entries per lane: 4 B of column and a value each, 48 KiB for the 1024 threads of the multi-level kernel in f64.  The
// long-row switch: a row of more than kIluSlice * L entries
constexpr uint32_t kIluSlice = 4;

// bad[0] = the smallest row whose columns are not strictly ascending, bad[1] = the smallest row without a stored (i, i)
__global__ void __launch_bounds__(kBlock)
k_ilu_check(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, uint64_t n, unsigned long long *bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        bool ascending = true, diag = false;
        const uint32_t k0 = off[i], k1 = off[i + 1];
        for (uint32_t k = k0; k < k1; ++k) {
            const uint32_t c = col[k];
            if (k > k0 && c <= col[k - 1]) ascending = false;
            if (c == i) diag = true;
        }
        if (!ascending) atomicMin(bad, (unsigned long long)i);
        if (!diag) atomicMin(bad + 1, (unsigned long long)i);
    }
}

// *diff != 0: the two patterns differ somewhere
__global__ void __launch_bounds__(kBlock)
k_ilu_same_pattern(const uint32_t *__restrict__ off_a, const uint32_t *__restrict__ off_b, uint64_t n_off, const uint32_t *__restrict__ col_a,
                   const uint32_t *__restrict__ col_b, uint64_t nnz, uint32_t *diff) {
    bool d = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_off; i += (uint64_t)gridDim.x * blockDim.x) d |= off_a[i] != off_b[i];
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (uint64_t)gridDim.x * blockDim.x) d |= col_a[i] != col_b[i];
    if (d) atomicOr(diff, 1u);
}

// w[k] of a row of an earlier level: as another wave of this workgroup may have stored it before the last barrier (MULTI)
template <typename T, bool MULTI> __device__ __forceinline__ T ilu_load(const T *w, uint32_t k) {
    if constexpr (MULTI) return __hip_atomic_load(w + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else return w[k];
}

// what the lanes of a group wrote before is what they read afterwards.  The group lies in one wavefront, whose LDS and vector memory
// operations are issued in program order: the fences keep the compiler from moving an access across, and (GLOBAL) order the
// vector memory operations at workgroup scope
template <bool GLOBAL> __device__ __forceinline__ void ilu_group_sync() {
    if constexpr (GLOBAL) {
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// the working row: in the group's LDS slice, or (LONG) in the value array itself
template <typename T, bool LONG> struct IluRow {
    const uint32_t *col;  // LONG: the row's columns in global memory; else the slice
    T *val;
    __device__ __forceinline__ uint32_t column(uint32_t p) const { return col[p]; }
    __device__ __forceinline__ T get(uint32_t p) const {
        if constexpr (LONG) return __hip_atomic_load(val + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else return val[p];
    }
    __device__ __forceinline__ void put(uint32_t p, T v) const {
        if constexpr (LONG) __hip_atomic_store(val + p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else val[p] = v;
    }
};

// the elimination steps of row i on `row` (len entries) by the L lanes of its group; returns the final diagonal value
template <typename T, int L, bool MULTI, bool LONG>
__device__ __forceinline__ T ilu_eliminate(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *w,
                                           const uint32_t *__restrict__ diagpos, uint32_t i, const IluRow<T, LONG> row, uint32_t len, uint32_t dpos) {
    const unsigned lane = threadIdx.x & (L - 1);
    for (uint32_t p = 0; p < len; ++p) {
        const uint32_t k = row.column(p);
        if (k >= i) break;  // (ascending columns: the strict lower part is done)
        const uint32_t dk = diagpos[k], ek = off[k + 1];
        const T q = p_div(row.get(p), ilu_load<T, MULTI>(w, dk));
        for (uint32_t jj = dk + 1 + lane; jj < ek; jj += L) {
            const uint32_t j = col[jj];
            uint32_t lo = p + 1, hi = len;  // (j > k: behind p)
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (row.column(mid) < j) lo = mid + 1;
                else hi = mid;
            }
            if (lo < len && row.column(lo) == j) row.put(lo, p_add(row.get(lo), -p_mul(q, ilu_load<T, MULTI>(w, jj))));
        }
        if (lane == 0) row.put(p, q);  // (every lane has read position p; no later step reads it)
        ilu_group_sync<LONG>();
    }
    return row.get(dpos);
}

// row i by the L lanes of its group (all of them arrive together); scol / sval: the group's slice of kIluSlice * L entries
template <typename T, int L, bool MULTI>
__device__ __forceinline__ void ilu_row(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, T *w, const uint32_t *__restrict__ diagpos,
                                        uint32_t i, uint32_t *scol, T *sval, unsigned long long *zero_pivot) {
    const unsigned lane = threadIdx.x & (L - 1);
    const uint32_t k0 = off[i], len = off[i + 1] - k0, dpos = diagpos[i] - k0;
    T d;
    if (len <= kIluSlice * L) {
        for (uint32_t p = lane; p < len; p += L) { scol[p] = col[k0 + p]; sval[p] = w[k0 + p]; }
        ilu_group_sync<false>();
        d = ilu_eliminate<T, L, MULTI, false>(off, col, w, diagpos, i, IluRow<T, false>{scol, sval}, len, dpos);
        for (uint32_t p = lane; p < len; p += L) w[k0 + p] = sval[p];
        ilu_group_sync<false>();  // (the slice is read before the group's next row overwrites it)
    } else {
        d = ilu_eliminate<T, L, MULTI, true>(off, col, w, diagpos, i, IluRow<T, true>{col + k0, w + k0}, len, dpos);
    }
    if (lane == 0 && d == T(0)) atomicMin(zero_pivot, (unsigned long long)i);
}

// MULTI = false: the rows rows[a .. e) of one level, a group each.  MULTI = true: one workgroup walks the levels [a, e), a barrier
// between them (which makes the values of a level visible to every wave of the workgroup before the next level reads them).
template <typename T, int L, bool MULTI>
__global__ void __launch_bounds__(MULTI ? (int)kTriSmallBlock : kBlock)
k_ilu_factor(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, T *w, const uint32_t *__restrict__ rows,
             const uint32_t *__restrict__ level_ptr, const uint32_t *__restrict__ diagpos, uint32_t a, uint32_t e, unsigned long long *zero_pivot) {
    constexpr uint32_t kThreads = MULTI ? kTriSmallBlock : (uint32_t)kBlock;
    __shared__ uint32_t s_col[kIluSlice * kThreads];
    __shared__ T s_val[kIluSlice * kThreads];
    const uint32_t g = threadIdx.x / L;
    uint32_t *scol = s_col + (size_t)g * kIluSlice * L;
    T *sval = s_val + (size_t)g * kIluSlice * L;
    if constexpr (MULTI) {
        const uint32_t groups = kTriSmallBlock / L;
        for (uint32_t lv = a; lv < e; ++lv) {
            const uint32_t r0 = level_ptr[lv], r1 = level_ptr[lv + 1];
            for (uint32_t q = r0 + g; q < r1; q += groups) ilu_row<T, L, true>(off, col, w, diagpos, rows[q], scol, sval, zero_pivot);
            __threadfence_block();
            __syncthreads();
        }
    } else {
        const uint64_t q = (uint64_t)a + ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / L;
        if (q < e) ilu_row<T, L, false>(off, col, w, diagpos, rows[q], scol, sval, zero_pivot);
    }
}

template <typename T, int L>
void ilu_launch(const smh_crs *f, const TriSchedule &t, const TriSchedule::Launch &l, unsigned long long *zero_pivot, hipStream_t s) {
    T *w = (T *)f->d_val;
    if (l.small) {
        hipLaunchKernelGGL((k_ilu_factor<T, L, true>), dim3(1), dim3(kTriSmallBlock), 0, s, f->d_off, f->d_col, w, t.rows.get(), t.level_ptr.get(),
                           t.diagpos.get(), l.level_begin, l.level_end, zero_pivot);
    } else {
        const uint64_t threads = (uint64_t)(l.row_end - l.row_begin) * L;
        hipLaunchKernelGGL((k_ilu_factor<T, L, false>), dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, f->d_off, f->d_col, w,
                           t.rows.get(), t.level_ptr.get(), t.diagpos.get(), l.row_begin, l.row_end, zero_pivot);
    }
}

template <typename T> int ilu_enqueue_t(const smh_crs *f, const TriSchedule &t, unsigned long long *zero_pivot, hipStream_t s) {
    const int lanes = tri_lanes(f);
    for (const TriSchedule::Launch &l : t.launches) {
        switch (lanes) {
        case 1: ilu_launch<T, 1>(f, t, l, zero_pivot, s); break;
        case 2: ilu_launch<T, 2>(f, t, l, zero_pivot, s); break;
        case 4: ilu_launch<T, 4>(f, t, l, zero_pivot, s); break;
        case 8: ilu_launch<T, 8>(f, t, l, zero_pivot, s); break;
        case 16: ilu_launch<T, 16>(f, t, l, zero_pivot, s); break;
        case 32: ilu_launch<T, 32>(f, t, l, zero_pivot, s); break;
        default: ilu_launch<T, 64>(f, t, l, zero_pivot, s); break;
        }
    }
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

}  // namespace

// the requirements on a pattern (ilu0's, and fsai.hip's), in the order of the header's table; nothing is written
int smh::ilu_check(const smh_crs *a, const char *what) {
    if (a->n_rows != a->n_cols) return fail(SMH_ERR_NOT_SQUARE, "%s: the matrix is not square", what);
    if (a->orphans) return fail(SMH_ERR_INVALID, "%s: the handle holds an orphaned entry", what);
    SMH_TRY(columns_within_n_cols(a, what));
    if (!a->n_rows) return SMH_OK;
    unsigned long long bad[2] = {~0ull, ~0ull};
    const hipStream_t s = a->stream;
    SMH_TRY(read_back(bad, 2, s, [&](unsigned long long *d) -> int {
        SMH_HIP(hipMemsetAsync(d, 0xFF, 2 * sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_ilu_check, dim3(grid_for(a->n_rows, kBuildGrid)), dim3(kBlock), 0, s, a->d_off, a->d_col, (uint64_t)a->n_rows, d);
        SMH_HIP(hipGetLastError());
        return SMH_OK;
    }));
    if (bad[0] != ~0ull) return fail(SMH_ERR_INVALID, "%s: the columns of row %llu are not strictly ascending (sort_rows; no duplicates)", what, bad[0]);
    if (bad[1] != ~0ull) return fail(SMH_ERR_INVALID, "%s: no diagonal entry stored in row %llu", what, bad[1]);
    return SMH_OK;
}

namespace {

// f's values (a copy of A's) become the factor, by f's LOWER schedule on f's stream; the value-derived forms of f go
int ilu_factor(smh_crs *f, size_t *zero_pivot_out) {
    SMH_TRY(ensure_tri_schedule(f, SMH_TRI_LOWER));
    const hipStream_t s = f->stream;
    unsigned long long zp = ~0ull;
    SMH_TRY(read_back(&zp, 1, s, [&](unsigned long long *d) -> int {
        SMH_HIP(hipMemsetAsync(d, 0xFF, sizeof(unsigned long long), s));
        if (f->dtype == SMH_F64) return ilu_enqueue_t<double>(f, f->tri[SMH_TRI_LOWER], d, s);
        return ilu_enqueue_t<float>(f, f->tri[SMH_TRI_LOWER], d, s);
    }));
    invalidate(f, Changed::Values);
    if (f->codes.state != Form::NotTried && f->codes.direct) {  // (as smh_crs_update_values: the value dictionary described the old values)
        StreamCfg c;
        SMH_TRY(stream_cfg(f, &c, true));
    }
    if (zero_pivot_out) *zero_pivot_out = zp == ~0ull ? SIZE_MAX : (size_t)zp;
    return SMH_OK;
}

}  // namespace

extern "C" int smh_crs_ilu0(const smh_crs *a, smh_crs **f_out, size_t *zero_pivot_out) {
    if (!a || !f_out) return fail(SMH_ERR_INVALID, "NULL argument");
    *f_out = nullptr;
    SMH_TRY(ilu_check(a, "ilu0"));
    smh_crs *f = nullptr;
    SMH_TRY(smh_crs_clone(a, &f));
    const int rc = ilu_factor(f, zero_pivot_out);
    if (rc != SMH_OK) return keep_error(rc, [&] { (void)smh_crs_destroy(f); });
    *f_out = f;
    return SMH_OK;
}

extern "C" int smh_crs_ilu0_refactor(smh_crs *f, const smh_crs *a, size_t *zero_pivot_out) {
    if (!f || !a) return fail(SMH_ERR_INVALID, "NULL handle");
    if (f == a) return fail(SMH_ERR_INVALID, "ilu0_refactor: the factor and the matrix are the same handle");
    if (f->dtype != a->dtype) return fail(SMH_ERR_INVALID, "ilu0_refactor: the factor's dtype differs from the matrix's");
    if (f->device != a->device) return fail(SMH_ERR_INVALID, "ilu0_refactor: the factor and the matrix live on different devices");
    if (f->n_rows != a->n_rows || f->n_cols != a->n_cols) return fail(SMH_ERR_DIM_MISMATCH, "ilu0_refactor: the factor's dimensions differ from the matrix's");
    if (f->nnz != a->nnz) return fail(SMH_ERR_INVALID, "ilu0_refactor: the factor's pattern differs from the matrix's");
    SMH_TRY(ilu_check(a, "ilu0_refactor"));
    const hipStream_t s = f->stream;
    SMH_HIP(hipStreamSynchronize(a->stream));  // (a's arrays are read on f's stream)
    if (a->nnz) {
        uint32_t diff = 0;
        SMH_TRY(read_back(&diff, 1, s, [&](uint32_t *d) -> int {
            SMH_HIP(hipMemsetAsync(d, 0, sizeof(uint32_t), s));
            hipLaunchKernelGGL(k_ilu_same_pattern, dim3(grid_for(a->nnz, kBuildGrid)), dim3(kBlock), 0, s, f->d_off, a->d_off, (uint64_t)a->n_rows + 1, f->d_col,
                               a->d_col, (uint64_t)a->nnz, d);
            SMH_HIP(hipGetLastError());
            return SMH_OK;
        }));
        if (diff) return fail(SMH_ERR_INVALID, "ilu0_refactor: the factor's pattern differs from the matrix's");
        SMH_HIP(hipMemcpyAsync(f->d_val, a->d_val, a->nnz * dtype_size(a->dtype), hipMemcpyDeviceToDevice, s));
    }
    return ilu_factor(f, zero_pivot_out);
}
