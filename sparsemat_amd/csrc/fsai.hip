// fsai.hip -- the factorized sparse approximate inverse (Kolotilina and Yeremin) of a CRS handle on the pattern of its lower triangle,
// gfx950.  An EXTENSION: the reference has none.
//
// (G, G^T) = fsai(A): G is lower triangular on the stored (i, c) of A with c <= i, G^T G approximates A^-1 and diag(G A G^T) = 1 for
// an SPD A.  It is applied by two products, z = G^T (G r) (pcg.hip), where SGS and ILU(0) take two level-scheduled solves.
// The contract (every operation rounded once, nothing fused; rows strictly ascending, every (i, i) stored): for row i let
// J = (j_0 < ... < j_(m-1) = i) be its stored columns <= i and B the dense lower triangle B[p][q] (q <= p) = the stored entry
// (j_p, j_q) of row j_p, 0 where none is stored -- entries above A's diagonal are never read.
//   for k = 0 .. m-2:                                          (elimination, no pivoting)
//       for p = k+1 .. m-1:  l_p = B[p][k] / B[k][k]
//       for p = k+1 .. m-1, q = k+1 .. p:  B[p][q] = B[p][q] - l_p * B[q][k]      (B[q][k]: the undivided value)
//       for p = k+1 .. m-1:  B[p][k] = l_p
//   y_(m-1) = 1;  for p = m-2 .. 0:  s = 0;  for q = p+1 .. m-1 ascending:  s = s + B[q][p] * y_q;   y_p = -s
//   g = 1 / sqrt(B[m-1][m-1]);  G[i, j_p] = y_p * g
// *not_spd = the smallest row whose last pivot B[m-1][m-1] is not > 0 (its values are IEEE's).  A row with m > kFsaiMaxRow is refused.
//
// The build is n independent rows: count (m per row) -> scan -> emit (G's columns: a prefix of A's row) -> the rows, nothing on the
// host but the launches, no kernel waits for another workgroup.  A group of L lanes per row (L from the mean m, as tri_lanes from the
// mean row) holds B in its slice of the LDS, kFsaiSlice * L values; a row whose triangle does not fit goes on a list and to a
// workgroup of kFsaiLongBlock threads with B in global scratch.  Both run fsai_row: lane t of the team gathers and eliminates the rows
// p = t, t + size, ... of B -- every update of a step is independent, so any team gives the contract's bits --, and its first lane
// takes the back substitution's sums in the stated order.
#include "crs_forms.hpp"
#include "solver_tree.hpp"

#include <cmath>
#include <cstdint>

using namespace smh;

namespace {

constexpr uint32_t kFsaiMaxRow = 128;    // most entries of a row on or below the diagonal
constexpr uint32_t kFsaiSlice = 8;       // LDS values per lane: 16 KiB for the 256 threads of a workgroup in f64
constexpr uint32_t kFsaiLongBlock = 128; // threads of the workgroup of a long row (m - 1 <= 127 rows of B are updated per step)
constexpr uint32_t kFsaiLongGrid = 512;  // most workgroups (and scratch triangles) of the long-row kernel
constexpr uint32_t kFsaiMaxTri = kFsaiMaxRow * (kFsaiMaxRow + 1) / 2;

__device__ __forceinline__ uint32_t tri(uint32_t p, uint32_t q) { return p * (p + 1) / 2 + q; }
template <typename T> __device__ __forceinline__ T fsai_sqrt(T a) { return (T)sqrt((double)a); }  // (f64's sqrt rounds an f32 correctly too)

// glen[i] = m_i, the stored columns <= i of row i (ascending: a prefix of the row); glen[n] = 0; stats[0] = the largest m,
// stats[1] = the smallest row with m > kFsaiMaxRow
__global__ void __launch_bounds__(kBlock)
k_fsai_count(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, uint64_t n, uint32_t *__restrict__ glen, unsigned long long *stats) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t m = 0;
        if (i < n) {
            const uint32_t k0 = off[i], k1 = off[i + 1];
            while (k0 + m < k1 && col[k0 + m] <= i) ++m;
            atomicMax(stats, (unsigned long long)m);
            if (m > kFsaiMaxRow) atomicMin(stats + 1, (unsigned long long)i);
        }
        glen[i] = m;
    }
}

__global__ void __launch_bounds__(kBlock)
k_fsai_emit(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, uint64_t n, const uint32_t *__restrict__ goff, uint32_t *__restrict__ gcol) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t k0 = off[i], g0 = goff[i], m = goff[i + 1] - g0;
        for (uint32_t p = 0; p < m; ++p) gcol[g0 + p] = col[k0 + p];
    }
}

// the rows whose triangle does not fit the slice (m > m_fit), in any order
__global__ void __launch_bounds__(kBlock)
k_fsai_long_list(const uint32_t *__restrict__ goff, uint64_t n, uint32_t m_fit, uint32_t *__restrict__ list, uint32_t *count) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (goff[i + 1] - goff[i] > m_fit) list[atomicAdd(count, 1u)] = (uint32_t)i;
}

// the L lanes of a row's group (part of one wavefront, whose LDS operations are issued in program order: the fences keep the compiler
// from moving an access across, as ilu.hip's)
template <int L> struct FsaiGroup {
    static constexpr uint32_t size = L;
    __device__ __forceinline__ static uint32_t rank() { return threadIdx.x & (L - 1); }
    __device__ __forceinline__ static void sync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};
// the workgroup of a long row; B is in global memory
struct FsaiBlock {
    static constexpr uint32_t size = kFsaiLongBlock;
    __device__ __forceinline__ static uint32_t rank() { return threadIdx.x; }
    __device__ __forceinline__ static void sync() {
        __threadfence_block();
        __syncthreads();
    }
};

// row i of G by a team that arrives together: J = gcol[0 .. m) its columns, B: room for m (m + 1) / 2 values, gval[0 .. m) the result
template <typename T, typename Team>
__device__ __forceinline__ void fsai_row(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val,
                                         const uint32_t *__restrict__ J, uint32_t m, uint32_t i, T *B, T *__restrict__ gval, unsigned long long *not_spd) {
    const uint32_t t = Team::rank();
    for (uint32_t p = t; p < m; p += Team::size) {
        const uint32_t r0 = off[J[p]], r1 = off[J[p] + 1];
        for (uint32_t q = 0; q <= p; ++q) {
            const uint32_t c = J[q];
            uint32_t lo = r0, hi = r1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (col[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            B[tri(p, q)] = lo < r1 && col[lo] == c ? val[lo] : T(0);
        }
    }
    Team::sync();
    for (uint32_t k = 0; k + 1 < m; ++k) {
        const T piv = B[tri(k, k)];
        for (uint32_t p = k + 1 + t; p < m; p += Team::size) {
            const T l = p_div(B[tri(p, k)], piv);
            for (uint32_t q = k + 1; q <= p; ++q) B[tri(p, q)] = p_add(B[tri(p, q)], -p_mul(l, B[tri(q, k)]));
        }
        Team::sync();  // (column k was read undivided by every lane)
        for (uint32_t p = k + 1 + t; p < m; p += Team::size) B[tri(p, k)] = p_div(B[tri(p, k)], piv);  // (no later step reads column k)
    }
    Team::sync();
    if (t == 0) {
        const T d = B[tri(m - 1, m - 1)];
        for (uint32_t p = m - 1; p-- > 0;) {  // y_p takes the place of the pivot B[p][p]
            T s = T(0);
            for (uint32_t q = p + 1; q < m; ++q) s = p_add(s, p_mul(B[tri(q, p)], q + 1 == m ? T(1) : B[tri(q, q)]));
            B[tri(p, p)] = -s;
        }
        const T g = p_div(T(1), fsai_sqrt(d));
        for (uint32_t p = 0; p < m; ++p) gval[p] = p_mul(p + 1 == m ? T(1) : B[tri(p, p)], g);
        if (!(d > T(0))) atomicMin(not_spd, (unsigned long long)i);
    }
    Team::sync();  // (B is read before the team's next row overwrites it)
}

// a group of L lanes per row; rows of more than m_fit entries are the long kernel's
template <typename T, int L>
__global__ void __launch_bounds__(kBlock)
k_fsai_rows(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val, const uint32_t *__restrict__ goff,
            const uint32_t *__restrict__ gcol, T *__restrict__ gval, uint64_t n, uint32_t m_fit, unsigned long long *not_spd) {
    __shared__ T s_b[kFsaiSlice * kBlock];
    const uint64_t i = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / L;
    if (i >= n) return;
    const uint32_t g0 = goff[i], m = goff[i + 1] - g0;
    if (m > m_fit) return;
    fsai_row<T, FsaiGroup<L>>(off, col, val, gcol + g0, m, (uint32_t)i, s_b + (size_t)(threadIdx.x / L) * kFsaiSlice * L, gval + g0, not_spd);
}

// a workgroup per listed row, B in the workgroup's kFsaiMaxTri values of scratch
template <typename T>
__global__ void __launch_bounds__(kFsaiLongBlock)
k_fsai_long(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val, const uint32_t *__restrict__ goff,
            const uint32_t *__restrict__ gcol, T *__restrict__ gval, const uint32_t *__restrict__ list, uint32_t n_long, T *scratch,
            unsigned long long *not_spd) {
    T *B = scratch + (size_t)blockIdx.x * kFsaiMaxTri;
    for (uint32_t q = blockIdx.x; q < n_long; q += gridDim.x) {
        const uint32_t i = list[q], g0 = goff[i], m = goff[i + 1] - g0;
        fsai_row<T, FsaiBlock>(off, col, val, gcol + g0, m, i, B, gval + g0, not_spd);
    }
}

// lanes per row: the smallest power of two that holds the mean m (smh_crs_set_vector_lanes on a overrides it, as for ilu0)
int fsai_lanes(const smh_crs *a, uint64_t nnz_g) {
    if (a->knobs.forced_lanes) return a->knobs.forced_lanes;
    const double mean = a->n_rows ? (double)nnz_g / (double)a->n_rows : 0.0;  // (a factor of a's transposition has a's rows too)
    int lanes = 1;
    while (lanes < kWave && (double)lanes < mean) lanes <<= 1;
    return lanes;
}
// the longest row whose triangle fits the slice of a group of `lanes` lanes
uint32_t fsai_fit(int lanes) {
    uint32_t m = 1;
    while ((m + 1) * (m + 2) / 2 <= kFsaiSlice * (uint32_t)lanes) ++m;
    return m;
}

template <typename T, int L>
void fsai_launch_rows(const smh_crs *a, const CrsArrays &g, uint64_t n, uint32_t m_fit, unsigned long long *not_spd, hipStream_t s) {
    const uint64_t blocks = (n * L + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((k_fsai_rows<T, L>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a->d_off, a->d_col, (const T *)a->d_val, g.off, g.col, (T *)g.val, n,
                       m_fit, not_spd);
}

// the values of G (offsets and columns are there) on s; d_not_spd: one word
template <typename T>
int fsai_values_t(const smh_crs *a, const CrsArrays &g, uint64_t nnz_g, uint32_t max_m, unsigned long long *d_not_spd, hipStream_t s) {
    const uint64_t n = a->n_rows;
    const int lanes = fsai_lanes(a, nnz_g);
    const uint32_t m_fit = fsai_fit(lanes);
    switch (lanes) {
    case 1: fsai_launch_rows<T, 1>(a, g, n, m_fit, d_not_spd, s); break;
    case 2: fsai_launch_rows<T, 2>(a, g, n, m_fit, d_not_spd, s); break;
    case 4: fsai_launch_rows<T, 4>(a, g, n, m_fit, d_not_spd, s); break;
    case 8: fsai_launch_rows<T, 8>(a, g, n, m_fit, d_not_spd, s); break;
    case 16: fsai_launch_rows<T, 16>(a, g, n, m_fit, d_not_spd, s); break;
    case 32: fsai_launch_rows<T, 32>(a, g, n, m_fit, d_not_spd, s); break;
    default: fsai_launch_rows<T, 64>(a, g, n, m_fit, d_not_spd, s); break;
    }
    SMH_HIP(hipGetLastError());
    if (max_m <= m_fit) return SMH_OK;
    Scratch scr;
    uint32_t *list = nullptr, *d_count = nullptr, n_long = 0;
    SMH_TRY(scr.alloc(&list, n));
    SMH_TRY(scr.alloc(&d_count, 1));
    SMH_TRY(read_back(d_count, &n_long, 1, s, [&](uint32_t *d) -> int {
        SMH_HIP(hipMemsetAsync(d, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_fsai_long_list, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, g.off, n, m_fit, list, d);
        SMH_HIP(hipGetLastError());
        return SMH_OK;
    }));
    const uint32_t grid = n_long < kFsaiLongGrid ? n_long : kFsaiLongGrid;
    T *tri_scratch = nullptr;
    SMH_TRY(scr.alloc(&tri_scratch, (size_t)grid * kFsaiMaxTri));
    hipLaunchKernelGGL((k_fsai_long<T>), dim3(grid), dim3(kFsaiLongBlock), 0, s, a->d_off, a->d_col, (const T *)a->d_val, g.off, g.col, (T *)g.val, list, n_long,
                       tri_scratch, d_not_spd);
    SMH_HIP(hipGetLastError());
    SMH_HIP(hipStreamSynchronize(s));  // (before the scratch goes back to the pool)
    return SMH_OK;
}

// ---- the non-symmetric FSAI (smh_crs_fsai_ns): the scheme above with B the full square ------------------------------------------------
// M^-1 = G_U G_L ~ A^-1.  The row solve R(C, i) on a CRS matrix C with ascending rows: J as above, B the dense m x m matrix
// B[p][q] = the stored entry (j_p, j_q) of C, 0 where none is stored -- both triangles --, every operation rounded once, nothing fused:
//   for k = 0 .. m-2:                                          (elimination, no pivoting)
//       for p = k+1 .. m-1:  l_p = B[p][k] / B[k][k]
//       for p = k+1 .. m-1, q = k+1 .. m-1:  B[p][q] = B[p][q] - l_p * B[k][q]
//       for p = k+1 .. m-1:  B[p][k] = l_p
//   y_(m-1) = 1;  for p = m-2 .. 0:  s = 0;  for q = p+1 .. m-1 ascending:  s = s + B[q][p] * y_q;   y_p = -s
//   d = B[m-1][m-1]                                            (d * the last row of B^-1 = y)
// Row i of G_L is y of R(A, i): a stored unit diagonal, G_L ~ L^-1 of A = L D U.  Row i of H is y / d of R(A^T, i), one division per
// entry, A^T with its rows ascending; G_U is the transposition of H as smh_crs_transpose stores it (n = 1: a copy).  For a dense
// pattern G_U G_L = A^-1.  *singular = the smallest row whose d, in either solve, is zero or not finite (the values are IEEE's).
// A step reads row k, which the step before finished, and writes rows p > k, each by the lane that owns it: one barrier per step.
// The slice of a group of L lanes is kFsaiNsSlice * L values and holds a square of m <= 4, 5, 8, 11, 16, 22, 32 for L = 1 .. 64.
constexpr uint32_t kFsaiNsSlice = 16;      // LDS values per lane: 32 KiB for the 256 threads of a workgroup in f64
constexpr uint32_t kFsaiNsLongGrid = 256;  // most workgroups (and scratch squares: kFsaiMaxRow^2 values each) of the long-row kernel

// row i of G_L (DIVIDE false) or of H (true) by a team that arrives together: J = gcol[0 .. m) its columns, B: room for m * m values
template <typename T, typename Team>
__device__ __forceinline__ void fsai_ns_row(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val,
                                            const uint32_t *__restrict__ J, uint32_t m, uint32_t i, T *B, T *__restrict__ gval, bool divide,
                                            unsigned long long *singular) {
    const uint32_t t = Team::rank();
    for (uint32_t p = t; p < m; p += Team::size) {
        const uint32_t r0 = off[J[p]], r1 = off[J[p] + 1];
        for (uint32_t q = 0; q < m; ++q) {
            const uint32_t c = J[q];
            uint32_t lo = r0, hi = r1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (col[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            B[p * m + q] = lo < r1 && col[lo] == c ? val[lo] : T(0);
        }
    }
    Team::sync();
    for (uint32_t k = 0; k + 1 < m; ++k) {
        const T piv = B[k * m + k];
        for (uint32_t p = k + 1 + t; p < m; p += Team::size) {
            const T l = p_div(B[p * m + k], piv);
            for (uint32_t q = k + 1; q < m; ++q) B[p * m + q] = p_add(B[p * m + q], -p_mul(l, B[k * m + q]));
            B[p * m + k] = l;
        }
        Team::sync();  // (row k + 1 is complete before it is read)
    }
    if (t == 0) {
        const T d = B[(m - 1) * m + m - 1];
        for (uint32_t p = m - 1; p-- > 0;) {  // y_p takes the place of the pivot B[p][p]
            T s = T(0);
            for (uint32_t q = p + 1; q < m; ++q) s = p_add(s, p_mul(B[q * m + p], q + 1 == m ? T(1) : B[q * m + q]));
            B[p * m + p] = -s;
        }
        for (uint32_t p = 0; p < m; ++p) {
            const T y = p + 1 == m ? T(1) : B[p * m + p];
            gval[p] = divide ? p_div(y, d) : y;
        }
        if (!(d != T(0) && isfinite(d))) atomicMin(singular, (unsigned long long)i);
    }
    Team::sync();  // (B is read before the team's next row overwrites it)
}

template <typename T, int L>
__global__ void __launch_bounds__(kBlock)
k_fsai_ns_rows(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val, const uint32_t *__restrict__ goff,
               const uint32_t *__restrict__ gcol, T *__restrict__ gval, uint64_t n, uint32_t m_fit, bool divide, unsigned long long *singular) {
    __shared__ T s_b[kFsaiNsSlice * kBlock];
    const uint64_t i = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / L;
    if (i >= n) return;
    const uint32_t g0 = goff[i], m = goff[i + 1] - g0;
    if (m > m_fit) return;
    fsai_ns_row<T, FsaiGroup<L>>(off, col, val, gcol + g0, m, (uint32_t)i, s_b + (size_t)(threadIdx.x / L) * kFsaiNsSlice * L, gval + g0, divide, singular);
}

template <typename T>
__global__ void __launch_bounds__(kFsaiLongBlock)
k_fsai_ns_long(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val, const uint32_t *__restrict__ goff,
               const uint32_t *__restrict__ gcol, T *__restrict__ gval, const uint32_t *__restrict__ list, uint32_t n_long, T *scratch, bool divide,
               unsigned long long *singular) {
    T *B = scratch + (size_t)blockIdx.x * kFsaiMaxRow * kFsaiMaxRow;
    for (uint32_t q = blockIdx.x; q < n_long; q += gridDim.x) {
        const uint32_t i = list[q], g0 = goff[i], m = goff[i + 1] - g0;
        fsai_ns_row<T, FsaiBlock>(off, col, val, gcol + g0, m, i, B, gval + g0, divide, singular);
    }
}

// the longest row whose square fits the slice of a group of `lanes` lanes
uint32_t fsai_ns_fit(int lanes) {
    uint32_t m = 1;
    while ((m + 1) * (m + 1) <= kFsaiNsSlice * (uint32_t)lanes) ++m;
    return m;
}

template <typename T, int L>
void fsai_ns_launch_rows(const smh_crs *c, const CrsArrays &g, uint64_t n, uint32_t m_fit, bool divide, unsigned long long *singular, hipStream_t s) {
    const uint64_t blocks = (n * L + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((k_fsai_ns_rows<T, L>), dim3((unsigned)blocks), dim3(kBlock), 0, s, c->d_off, c->d_col, (const T *)c->d_val, g.off, g.col, (T *)g.val, n,
                       m_fit, divide, singular);
}

// the values of a factor of c (offsets and columns are there) on s; d_singular: one word, shared by both factors.  lanes_of: the handle
// whose smh_crs_set_vector_lanes counts (a itself, also for the rows of its transposition)
template <typename T>
int fsai_ns_values_t(const smh_crs *c, const smh_crs *lanes_of, const CrsArrays &g, uint64_t nnz_g, uint32_t max_m, bool divide,
                     unsigned long long *d_singular, hipStream_t s) {
    const uint64_t n = c->n_rows;
    const int lanes = fsai_lanes(lanes_of, nnz_g);
    const uint32_t m_fit = fsai_ns_fit(lanes);
    switch (lanes) {
    case 1: fsai_ns_launch_rows<T, 1>(c, g, n, m_fit, divide, d_singular, s); break;
    case 2: fsai_ns_launch_rows<T, 2>(c, g, n, m_fit, divide, d_singular, s); break;
    case 4: fsai_ns_launch_rows<T, 4>(c, g, n, m_fit, divide, d_singular, s); break;
    case 8: fsai_ns_launch_rows<T, 8>(c, g, n, m_fit, divide, d_singular, s); break;
    case 16: fsai_ns_launch_rows<T, 16>(c, g, n, m_fit, divide, d_singular, s); break;
    case 32: fsai_ns_launch_rows<T, 32>(c, g, n, m_fit, divide, d_singular, s); break;
    default: fsai_ns_launch_rows<T, 64>(c, g, n, m_fit, divide, d_singular, s); break;
    }
    SMH_HIP(hipGetLastError());
    if (max_m <= m_fit) return SMH_OK;
    Scratch scr;
    uint32_t *list = nullptr, *d_count = nullptr, n_long = 0;
    SMH_TRY(scr.alloc(&list, n));
    SMH_TRY(scr.alloc(&d_count, 1));
    SMH_TRY(read_back(d_count, &n_long, 1, s, [&](uint32_t *d) -> int {
        SMH_HIP(hipMemsetAsync(d, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_fsai_long_list, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, g.off, n, m_fit, list, d);
        SMH_HIP(hipGetLastError());
        return SMH_OK;
    }));
    const uint32_t grid = n_long < kFsaiNsLongGrid ? n_long : kFsaiNsLongGrid;
    T *sq_scratch = nullptr;
    SMH_TRY(scr.alloc(&sq_scratch, (size_t)grid * kFsaiMaxRow * kFsaiMaxRow));
    hipLaunchKernelGGL((k_fsai_ns_long<T>), dim3(grid), dim3(kFsaiLongBlock), 0, s, c->d_off, c->d_col, (const T *)c->d_val, g.off, g.col, (T *)g.val, list,
                       n_long, sq_scratch, divide, d_singular);
    SMH_HIP(hipGetLastError());
    SMH_HIP(hipStreamSynchronize(s));  // (before the scratch goes back to the pool)
    return SMH_OK;
}

// count -> scan: the offsets of a factor on c's stored (i, col <= i); stats[0] = the largest m, stats[1] = the smallest row with
// m > kFsaiMaxRow (the caller's to refuse), *nnz_g = the entries
int fsai_ns_offsets(const smh_crs *c, CrsArrays &g, unsigned long long stats[2], uint64_t *nnz_g, hipStream_t s) {
    const size_t n = c->n_rows;
    SMH_TRY(g.alloc_off(n));
    stats[0] = 0;
    stats[1] = ~0ull;
    SMH_TRY(read_back(stats, 2, s, [&](unsigned long long *d) -> int {
        SMH_HIP(hipMemcpyAsync(d, stats, 2 * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fsai_count, dim3(grid_for(n + 1, kBuildGrid)), dim3(kBlock), 0, s, c->d_off, c->d_col, (uint64_t)n, g.off, d);
        SMH_HIP(hipGetLastError());
        return SMH_OK;
    }));
    if (stats[1] != ~0ull) return SMH_OK;
    SMH_TRY(device_exclusive_scan_u32(g.off, (uint64_t)n + 1, s, nnz_g));
    if (*nnz_g >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    return SMH_OK;
}

// emit -> the rows: the columns and values of a factor of c whose offsets are there
int fsai_ns_fill(const smh_crs *c, const smh_crs *lanes_of, CrsArrays &g, uint64_t nnz_g, uint32_t max_m, bool divide, unsigned long long *d_singular,
                 hipStream_t s) {
    const size_t n = c->n_rows, vs = dtype_size(c->dtype);
    SMH_TRY(g.alloc_entries(nnz_g, vs));
    SMH_TRY(g.zero_padding(nnz_g, vs, s));
    if (!n) return SMH_OK;
    hipLaunchKernelGGL(k_fsai_emit, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, c->d_off, c->d_col, (uint64_t)n, g.off, g.col);
    SMH_HIP(hipGetLastError());
    if (c->dtype == SMH_F64) return fsai_ns_values_t<double>(c, lanes_of, g, nnz_g, max_m, divide, d_singular, s);
    return fsai_ns_values_t<float>(c, lanes_of, g, nnz_g, max_m, divide, d_singular, s);
}

// a 1 x 1 matrix is its own transpose (the transposition's replay of one operation would leave an orphan and no row)
int fsai_transpose(const smh_crs *h, smh_crs **out) { return h->nnz == 1 ? smh_crs_clone(h, out) : smh_crs_transpose(h, out); }

}  // namespace

extern "C" int smh_crs_fsai(const smh_crs *a, smh_crs **g_out, smh_crs **gt_out, size_t *not_spd_out) {
    if (!a || !g_out || !gt_out) return fail(SMH_ERR_INVALID, "NULL argument");
    *g_out = *gt_out = nullptr;
    SMH_TRY(ilu_check(a, "fsai"));
    const size_t n = a->n_rows, vs = dtype_size(a->dtype);
    const hipStream_t s = a->stream;
    CrsArrays g;
    SMH_TRY(g.alloc_off(n));
    // count -> scan -> emit: the pattern of G
    unsigned long long stats[2] = {0, ~0ull};
    SMH_TRY(read_back(stats, 2, s, [&](unsigned long long *d) -> int {
        SMH_HIP(hipMemcpyAsync(d, stats, sizeof stats, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fsai_count, dim3(grid_for(n + 1, kBuildGrid)), dim3(kBlock), 0, s, a->d_off, a->d_col, (uint64_t)n, g.off, d);
        SMH_HIP(hipGetLastError());
        return SMH_OK;
    }));
    if (stats[1] != ~0ull)
        return fail(SMH_ERR_INVALID, "fsai: row %llu stores more than %u entries on or below the diagonal", stats[1], kFsaiMaxRow);
    uint64_t nnz_g = 0;
    SMH_TRY(device_exclusive_scan_u32(g.off, (uint64_t)n + 1, s, &nnz_g));
    if (nnz_g >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    SMH_TRY(g.alloc_entries(nnz_g, vs));
    SMH_TRY(g.zero_padding(nnz_g, vs, s));
    unsigned long long not_spd = ~0ull;
    if (n) {
        hipLaunchKernelGGL(k_fsai_emit, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, a->d_off, a->d_col, (uint64_t)n, g.off, g.col);
        SMH_HIP(hipGetLastError());
        SMH_TRY(read_back(&not_spd, 1, s, [&](unsigned long long *d) -> int {
            SMH_HIP(hipMemsetAsync(d, 0xFF, sizeof(unsigned long long), s));
            if (a->dtype == SMH_F64) return fsai_values_t<double>(a, g, nnz_g, (uint32_t)stats[0], d, s);
            return fsai_values_t<float>(a, g, nnz_g, (uint32_t)stats[0], d, s);
        }));
    }
    SMH_HIP(hipStreamSynchronize(s));  // (the new handles have streams of their own)
    smh_crs *gh = nullptr, *gth = nullptr;
    SMH_TRY(wrap_arrays(a->dtype, nullptr, n, n, nnz_g, g, 0, &gh));
    // (n = 1: the transposition replays one operation, which the reference's container leaves as an orphan without a row; a 1 x 1
    // matrix is its own transpose)
    const int rc = nnz_g == 1 ? smh_crs_clone(gh, &gth) : smh_crs_transpose(gh, &gth);
    if (rc != SMH_OK) return keep_error(rc, [&] { (void)smh_crs_destroy(gh); });
    *g_out = gh;
    *gt_out = gth;
    if (not_spd_out) *not_spd_out = not_spd == ~0ull ? SIZE_MAX : (size_t)not_spd;
    return SMH_OK;
}

extern "C" int smh_crs_fsai_ns(const smh_crs *a, smh_crs **gl_out, smh_crs **gu_out, size_t *singular_out) {
    if (!a || !gl_out || !gu_out) return fail(SMH_ERR_INVALID, "NULL argument");
    *gl_out = *gu_out = nullptr;
    SMH_TRY(ilu_check(a, "fsai_ns"));
    const size_t n = a->n_rows;
    const hipStream_t s = a->stream;
    // A^T with its rows ascending (the library's transposition stores them descending), on a stream of its own
    smh_crs *at = nullptr;
    SMH_TRY(fsai_transpose(a, &at));
    struct Drop {  // (destroying a handle leaves the last error's text alone)
        smh_crs *h;
        ~Drop() { (void)smh_crs_destroy(h); }
    } drop_at{at};
    SMH_TRY(smh_crs_sort_rows(at));
    SMH_HIP(hipStreamSynchronize(at->stream));  // (it is read on a's stream)
    // the patterns of both factors, and their refusals, before either's values
    CrsArrays gl, h;
    unsigned long long stats_l[2], stats_u[2];
    uint64_t nnz_l = 0, nnz_u = 0;
    SMH_TRY(fsai_ns_offsets(a, gl, stats_l, &nnz_l, s));
    if (stats_l[1] != ~0ull)
        return fail(SMH_ERR_INVALID, "fsai_ns: row %llu stores more than %u entries on or below the diagonal", stats_l[1], kFsaiMaxRow);
    SMH_TRY(fsai_ns_offsets(at, h, stats_u, &nnz_u, s));
    if (stats_u[1] != ~0ull)
        return fail(SMH_ERR_INVALID, "fsai_ns: column %llu stores more than %u entries on or above the diagonal", stats_u[1], kFsaiMaxRow);
    unsigned long long singular = ~0ull;
    SMH_TRY(read_back(&singular, 1, s, [&](unsigned long long *d) -> int {
        SMH_HIP(hipMemsetAsync(d, 0xFF, sizeof(unsigned long long), s));
        SMH_TRY(fsai_ns_fill(a, a, gl, nnz_l, (uint32_t)stats_l[0], /*divide*/ false, d, s));
        return fsai_ns_fill(at, a, h, nnz_u, (uint32_t)stats_u[0], /*divide*/ true, d, s);
    }));
    SMH_HIP(hipStreamSynchronize(s));  // (the new handles have streams of their own)
    smh_crs *glh = nullptr, *hh = nullptr, *guh = nullptr;
    SMH_TRY(wrap_arrays(a->dtype, nullptr, n, n, nnz_l, gl, 0, &glh));
    int rc = wrap_arrays(a->dtype, nullptr, n, n, nnz_u, h, 0, &hh);
    if (rc == SMH_OK) {
        rc = fsai_transpose(hh, &guh);
        rc = keep_error(rc, [&] { (void)smh_crs_destroy(hh); });
    }
    if (rc != SMH_OK) return keep_error(rc, [&] { (void)smh_crs_destroy(glh); });
    *gl_out = glh;
    *gu_out = guh;
    if (singular_out) *singular_out = singular == ~0ull ? SIZE_MAX : (size_t)singular;
    return SMH_OK;
}
