// trisolve.hip -- sparse triangular solves on a CRS handle by level scheduling, gfx950.  An EXTENSION: the reference has none.
//
// The dependency of row i is every stored column c < i (LOWER) or c > i (UPPER); level(i) = 0 without one, else 1 + max level(c).
// Rows of one level are independent, so a level is one gather sweep over its row list.  The schedule (TriSchedule, internal.hpp) is a
// derived form of the handle, one per uplo: the rows level by level, the position of every row's first stored (i, i), and the launch
// plan.  It holds positions only: new values leave it valid, a new storage order or new arrays drop it.
//
// Build: rounds of one kernel.  Round k gives level k to every row without a level whose dependencies all got theirs in an EARLIER
// round (a level read as "none" or as k itself fails the test alike, so rows that race inside a round cannot see each other), and
// counts them; the host reads the counts a batch of rounds at a time and stops when every row has a level.  One launch per level
// and n + (entries of the rows still without a level) words read per round; a stable radix sort by level then lists the rows.
//
// Solve: a level of more than kTriSmallRows rows is one launch on a grid.  A run of consecutive levels of at most that many rows each
// is ONE launch of one workgroup that walks them with a workgroup barrier between levels (a bidiagonal chain of n rows: one launch).
// No kernel waits for a value another workgroup writes.  A lane group per row (width from the mean row length, as K1's): each lane
// loads one entry of a pass coalesced and rounds its product val[k] * x[c]; the group's first lane then subtracts the products in
// storage order, one rounding each -- the sequential definition bit for bit at every width:
//   s = b[i];  for k in storage order: c = col[k]; if c in the triangle: s = s - val[k] * x[c];  x[i] = NON_UNIT ? s / val[diagpos[i]] : s
#include <rocprim/device/device_radix_sort.hpp>

#include <cstdlib>

#include "crs_forms.hpp"
#include "solver_tree.hpp"

using namespace smh;

namespace {

constexpr uint32_t kNoLevel = 0xFFFFFFFFu;

__device__ __forceinline__ bool tri_depends(uint32_t c, uint32_t i, int upper) { return upper ? c > i : c < i; }

// one round of the level build; cnt[round] += rows that got level `round`
__global__ void __launch_bounds__(kBlock)
k_tri_round(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, uint64_t n, int upper, uint32_t round, uint32_t *level, uint32_t *cnt) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        bool take = level[i] == kNoLevel;
        if (take) {
            for (uint32_t k = off[i]; k < off[i + 1]; ++k) {
                const uint32_t c = col[k];
                if (tri_depends(c, (uint32_t)i, upper) && level[c] >= round) { take = false; break; }
            }
        }
        if (take) level[i] = round;
        const unsigned long long taken = __ballot(take);
        if (take && (int)(threadIdx.x & (kWave - 1)) == __ffsll((long long)taken) - 1) atomicAdd(cnt + round, (uint32_t)__popcll(taken));
    }
}

// diagpos[i] = the first k with col[k] == i (~0u: none); *bad = the smallest row without one
__global__ void __launch_bounds__(kBlock)
k_tri_diagpos(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, uint64_t n, uint32_t *__restrict__ diagpos, unsigned long long *bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t pos = ~0u;
        for (uint32_t k = off[i]; k < off[i + 1]; ++k)
            if (col[k] == i) { pos = k; break; }
        diagpos[i] = pos;
        if (pos == ~0u) atomicMin(bad, (unsigned long long)i);
    }
}

__global__ void __launch_bounds__(kBlock) k_tri_iota(uint32_t *out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = (uint32_t)i;
}

// x[c] as another wave of this workgroup may have stored it before the last barrier: never a value the compiler kept from before
template <typename T, bool MULTI> __device__ __forceinline__ T tri_load_x(const T *x, uint32_t c) {
    if constexpr (MULTI) return __hip_atomic_load(x + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else return x[c];
}

// row i by the L lanes of its group (all of them arrive together); the group's lane 0 stores x[i]
template <typename T, int L, bool MULTI>
__device__ __forceinline__ void tri_row(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val,
                                        const uint32_t *__restrict__ diagpos, const T *b, T *x, uint32_t i, int upper, int unit, int scale_rhs) {
    const unsigned lane = threadIdx.x & (L - 1);
    const uint32_t k0 = off[i], k1 = off[i + 1];
    T s = T(0);
    if (lane == 0) {
        s = b[i];
        if (scale_rhs) s = p_mul(s, val[diagpos[i]]);
    }
    for (uint32_t base = k0; base < k1; base += L) {
        const uint32_t k = base + lane;
        bool use = false;
        T pr = T(0);
        if (k < k1) {
            const uint32_t c = col[k];
            use = tri_depends(c, i, upper);
            if (use) pr = p_mul(val[k], tri_load_x<T, MULTI>(x, c));
        }
        if constexpr (L == 1) {
            if (use) s = p_add(s, -pr);
        } else {
            // the group's share of the wave's ballot, then its products one by one to lane 0, in storage order
            const unsigned long long all = __ballot(use);
            const unsigned first = (threadIdx.x & (kWave - 1)) & ~(unsigned)(L - 1);
            const unsigned long long mine = L == kWave ? all : (all >> first) & ((1ull << (L & 63)) - 1ull);
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const T pj = (T)__shfl(pr, j, L);
                if ((mine >> j) & 1ull) s = p_add(s, -pj);
            }
        }
    }
    if (lane == 0) x[i] = unit ? s : p_div(s, val[diagpos[i]]);
}

// MULTI = false: the rows rows[a .. e) of one level, a group each.  MULTI = true: one workgroup walks the levels [a, e), a barrier
// between them (which makes the x of a level visible to every wave of the workgroup before the next level reads it).
template <typename T, int L, bool MULTI>
__global__ void __launch_bounds__(MULTI ? (int)kTriSmallBlock : kBlock)
k_tri_solve(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val, const uint32_t *__restrict__ rows,
            const uint32_t *__restrict__ level_ptr, const uint32_t *__restrict__ diagpos, uint32_t a, uint32_t e, const T *b, T *x, int upper, int unit,
            int scale_rhs, const uint32_t *active) {
    if (active && !*active) return;  // (uniform over the launch)
    if constexpr (MULTI) {
        const uint32_t groups = kTriSmallBlock / L, g = threadIdx.x / L;
        for (uint32_t lv = a; lv < e; ++lv) {
            const uint32_t r0 = level_ptr[lv], r1 = level_ptr[lv + 1];
            for (uint32_t q = r0 + g; q < r1; q += groups) tri_row<T, L, true>(off, col, val, diagpos, b, x, rows[q], upper, unit, scale_rhs);
            __threadfence_block();
            __syncthreads();
        }
    } else {
        const uint64_t q = (uint64_t)a + ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / L;
        if (q < e) tri_row<T, L, false>(off, col, val, diagpos, b, x, rows[q], upper, unit, scale_rhs);
    }
}

template <typename T, int L>
void tri_launch(const smh_crs *m, const TriSchedule &t, const TriSchedule::Launch &l, const T *b, T *x, int upper, int unit, int scale_rhs,
                const uint32_t *active, hipStream_t s) {
    const T *val = (const T *)m->d_val;
    if (l.small) {
        hipLaunchKernelGGL((k_tri_solve<T, L, true>), dim3(1), dim3(kTriSmallBlock), 0, s, m->d_off, m->d_col, val, t.rows.get(), t.level_ptr.get(),
                           t.diagpos.get(), l.level_begin, l.level_end, b, x, upper, unit, scale_rhs, active);
    } else {
        const uint64_t threads = (uint64_t)(l.row_end - l.row_begin) * L;
        hipLaunchKernelGGL((k_tri_solve<T, L, false>), dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, m->d_off, m->d_col, val,
                           t.rows.get(), t.level_ptr.get(), t.diagpos.get(), l.row_begin, l.row_end, b, x, upper, unit, scale_rhs, active);
    }
}

template <typename T>
int trisolve_t(smh_crs *m, const TriSchedule &t, int upper, int unit, int scale_rhs, const T *b, T *x, const uint32_t *active, hipStream_t s) {
    const int lanes = tri_lanes(m);
    for (const TriSchedule::Launch &l : t.launches) {
        switch (lanes) {
        case 1: tri_launch<T, 1>(m, t, l, b, x, upper, unit, scale_rhs, active, s); break;
        case 2: tri_launch<T, 2>(m, t, l, b, x, upper, unit, scale_rhs, active, s); break;
        case 4: tri_launch<T, 4>(m, t, l, b, x, upper, unit, scale_rhs, active, s); break;
        case 8: tri_launch<T, 8>(m, t, l, b, x, upper, unit, scale_rhs, active, s); break;
        case 16: tri_launch<T, 16>(m, t, l, b, x, upper, unit, scale_rhs, active, s); break;
        case 32: tri_launch<T, 32>(m, t, l, b, x, upper, unit, scale_rhs, active, s); break;
        default: tri_launch<T, 64>(m, t, l, b, x, upper, unit, scale_rhs, active, s); break;
        }
    }
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

bool valid_uplo(int uplo) { return uplo == SMH_TRI_LOWER || uplo == SMH_TRI_UPPER; }

// the checks every entry point shares; the schedule exists afterwards
int tri_prepare(smh_crs *m, int uplo, const char *what) {
    if (!valid_uplo(uplo)) return fail(SMH_ERR_INVALID, "%s: uplo must be SMH_TRI_LOWER or SMH_TRI_UPPER", what);
    if (m->n_rows != m->n_cols) return fail(SMH_ERR_NOT_SQUARE, "%s: the matrix is not square", what);
    if (m->orphans) return fail(SMH_ERR_INVALID, "%s: the handle holds an orphaned entry", what);
    SMH_TRY(columns_within_n_cols(m, what));
    return ensure_tri_schedule(m, uplo);
}

int tri_check_solve(smh_crs *m, int uplo, int diag, const char *what) {
    if (diag != SMH_DIAG_NON_UNIT && diag != SMH_DIAG_UNIT) return fail(SMH_ERR_INVALID, "%s: diag must be SMH_DIAG_NON_UNIT or SMH_DIAG_UNIT", what);
    SMH_TRY(tri_prepare(m, uplo, what));
    if (diag == SMH_DIAG_NON_UNIT && m->tri[uplo].first_no_diag != ~0ull)
        return fail(SMH_ERR_INVALID, "%s: no diagonal entry stored in row %llu", what, (unsigned long long)m->tri[uplo].first_no_diag);
    return SMH_OK;
}

}  // namespace

namespace smh {

// lanes per row: the smallest power of two that holds the mean row in one pass (smh_crs_set_vector_lanes overrides it, as for K1)
int tri_lanes(const smh_crs *m) {
    if (m->knobs.forced_lanes) return m->knobs.forced_lanes;
    const double mean = m->n_rows ? (double)m->nnz / (double)m->n_rows : 0.0;
    int lanes = 1;
    while (lanes < kWave && (double)lanes < mean) lanes <<= 1;
    return lanes;
}

int ensure_tri_schedule(smh_crs *m, int uplo) {
    if (m->tri[uplo].state == Form::Ready) return SMH_OK;
    const size_t n = m->n_rows;
    const hipStream_t s = m->stream;
    TriSchedule t;
    std::vector<uint32_t> ptr(1, 0u);  // where each level starts
    try {
        if (n) {
            Scratch scr;
            uint32_t *cnt = nullptr, *iota = nullptr, *keys = nullptr;
            unsigned long long *d_bad = nullptr, bad = ~0ull;
            SMH_TRY(t.level.alloc(n));
            SMH_TRY(t.rows.alloc(n));
            SMH_TRY(t.diagpos.alloc(n));
            SMH_TRY(scr.alloc(&cnt, n));
            SMH_TRY(scr.alloc(&d_bad, 1));
            SMH_HIP(hipMemsetAsync(t.level.get(), 0xFF, n * sizeof(uint32_t), s));
            SMH_HIP(hipMemsetAsync(cnt, 0, n * sizeof(uint32_t), s));
            SMH_HIP(hipMemcpyAsync(d_bad, &bad, sizeof bad, hipMemcpyHostToDevice, s));
            const unsigned grid = grid_for(n, kBuildGrid);
            hipLaunchKernelGGL(k_tri_diagpos, dim3(grid), dim3(kBlock), 0, s, m->d_off, m->d_col, (uint64_t)n, t.diagpos.get(), d_bad);
            SMH_HIP(hipGetLastError());
            // every round gives at least one row its level (the first row without one in index order, LOWER; the last, UPPER), so `left`
            // rows need at most `left` more rounds and no round is numbered n or beyond
            std::vector<uint32_t> h_cnt;
            size_t done = 0, round = 0, batch = 4;
            while (done < n) {
                const size_t left = n - done, rounds = batch < left ? batch : left;
                for (size_t k = 0; k < rounds; ++k)
                    hipLaunchKernelGGL(k_tri_round, dim3(grid), dim3(kBlock), 0, s, m->d_off, m->d_col, (uint64_t)n, uplo == SMH_TRI_UPPER ? 1 : 0,
                                       (uint32_t)(round + k), t.level.get(), cnt);
                SMH_HIP(hipGetLastError());
                h_cnt.resize(rounds);
                SMH_HIP(hipMemcpyAsync(h_cnt.data(), cnt + round, rounds * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
                SMH_HIP(hipStreamSynchronize(s));
                for (size_t k = 0; k < rounds && done < n; ++k) {
                    if (h_cnt[k] == 0) return fail(SMH_ERR_INVALID, "trisolve: the level build made no progress in round %zu", round + k);
                    done += h_cnt[k];
                    ptr.push_back((uint32_t)done);
                }
                round += rounds;
                if (batch < 64) batch *= 2;
            }
            SMH_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
            // the rows level by level: a stable sort of 0 .. n-1 by level
            SMH_TRY(scr.alloc(&iota, n));
            SMH_TRY(scr.alloc(&keys, n));
            hipLaunchKernelGGL(k_tri_iota, dim3(grid), dim3(kBlock), 0, s, iota, (uint64_t)n);
            SMH_HIP(hipGetLastError());
            SMH_ROCPRIM(s, rocprim::radix_sort_pairs(tmp, bytes, t.level.get(), keys, iota, t.rows.get(), n, 0u, bits_for(ptr.size() - 1), s));
            t.first_no_diag = bad;
        }
        t.n_levels = ptr.size() - 1;
        SMH_TRY(t.level_ptr.alloc(ptr.size()));
        SMH_HIP(hipMemcpyAsync(t.level_ptr.get(), ptr.data(), ptr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        SMH_HIP(hipStreamSynchronize(s));
        // the launch plan
        for (size_t lv = 0; lv < t.n_levels;) {
            TriSchedule::Launch l;
            l.level_begin = (uint32_t)lv;
            l.row_begin = ptr[lv];
            l.small = ptr[lv + 1] - ptr[lv] <= kTriSmallRows;
            ++lv;
            while (l.small && lv < t.n_levels && ptr[lv + 1] - ptr[lv] <= kTriSmallRows) ++lv;
            l.level_end = (uint32_t)lv;
            l.row_end = ptr[lv];
            t.launches.push_back(l);
        }
    } catch (...) {
        return fail(SMH_ERR_OOM, "host allocation failed");
    }
    t.state = Form::Ready;
    m->tri[uplo] = std::move(t);
    return SMH_OK;
}

int trisolve_enqueue(smh_crs *m, int uplo, int diag, bool scale_rhs, const void *b, void *x, const uint32_t *active, hipStream_t s) {
    const TriSchedule &t = m->tri[uplo];
    const int upper = uplo == SMH_TRI_UPPER ? 1 : 0, unit = diag == SMH_DIAG_UNIT ? 1 : 0;
    if (m->dtype == SMH_F64) return trisolve_t<double>(m, t, upper, unit, scale_rhs ? 1 : 0, (const double *)b, (double *)x, active, s);
    return trisolve_t<float>(m, t, upper, unit, scale_rhs ? 1 : 0, (const float *)b, (float *)x, active, s);
}

}  // namespace smh

extern "C" int smh_crs_trisolve_levels(smh_crs *m, int uplo, size_t *n_levels_out, uint32_t *level_of_row_out, size_t *n_launches_out,
                                       size_t *small_level_rows_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(tri_prepare(m, uplo, "trisolve_levels"));
    const TriSchedule &t = m->tri[uplo];
    if (n_levels_out) *n_levels_out = t.n_levels;
    if (n_launches_out) *n_launches_out = t.launches.size();
    if (small_level_rows_out) *small_level_rows_out = kTriSmallRows;
    if (level_of_row_out && m->n_rows) SMH_HIP(hipMemcpy(level_of_row_out, t.level.get(), m->n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SMH_OK;
}

extern "C" int smh_crs_trisolve_vec(smh_crs *m, int uplo, int diag, const smh_vec *b, smh_vec *x) {
    if (!m || !b || !x) return fail(SMH_ERR_INVALID, "NULL handle");
    if (b->dtype != m->dtype || x->dtype != m->dtype) return fail(SMH_ERR_INVALID, "vector dtype differs from the matrix's");
    if (!valid_uplo(uplo)) return fail(SMH_ERR_INVALID, "trisolve: uplo must be SMH_TRI_LOWER or SMH_TRI_UPPER");
    if (m->n_rows != m->n_cols) return fail(SMH_ERR_NOT_SQUARE, "trisolve: the matrix is not square");
    if (m->n_rows != b->n || m->n_rows != x->n) return fail(SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch");
    const char *pb = (const char *)b->d, *px = (const char *)x->d;
    const size_t bytes = m->n_rows * dtype_size(m->dtype);
    if (pb != px && pb < px + bytes && px < pb + bytes) return fail(SMH_ERR_INVALID, "trisolve: b and x overlap in part");
    SMH_TRY(tri_check_solve(m, uplo, diag, "trisolve"));
    SMH_TRY(trisolve_enqueue(m, uplo, diag, false, b->d, x->d, nullptr, m->stream));
    SMH_HIP(hipStreamSynchronize(m->stream));
    return SMH_OK;
}

extern "C" int smh_crs_trisolve(smh_crs *m, int uplo, int diag, const void *b_host, size_t b_len, void *x_host, size_t x_len) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (!valid_uplo(uplo)) return fail(SMH_ERR_INVALID, "trisolve: uplo must be SMH_TRI_LOWER or SMH_TRI_UPPER");
    const size_t n = m->n_rows;
    if (n != m->n_cols) return fail(SMH_ERR_NOT_SQUARE, "trisolve: the matrix is not square");
    if (n != b_len || n != x_len) return fail(SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch");
    if (n && (!b_host || !x_host)) return fail(SMH_ERR_INVALID, "NULL host vector");
    const size_t bytes = n * dtype_size(m->dtype);
    const char *pb = (const char *)b_host, *px = (const char *)x_host;
    if (n && pb != px && pb < px + bytes && px < pb + bytes) return fail(SMH_ERR_INVALID, "trisolve: b and x overlap in part");
    SMH_TRY(tri_check_solve(m, uplo, diag, "trisolve"));
    if (!n) return SMH_OK;
    Scratch scr;
    char *d = nullptr;
    SMH_TRY(scr.alloc(&d, bytes));
    const hipStream_t s = m->stream;
    const int rc = [&]() -> int {
        SMH_HIP(hipMemcpyAsync(d, b_host, bytes, hipMemcpyHostToDevice, s));
        SMH_TRY(trisolve_enqueue(m, uplo, diag, false, d, d, nullptr, s));
        SMH_HIP(hipMemcpyAsync(x_host, d, bytes, hipMemcpyDeviceToHost, s));
        return SMH_OK;
    }();
    // the stream is drained before the scratch goes back to the pool, also after a failure
    if (rc != SMH_OK) return keep_error(rc, [&] { (void)hipStreamSynchronize(s); (void)hipGetLastError(); });
    SMH_HIP(hipStreamSynchronize(s));
    return SMH_OK;
}
