// permute.hip -- row / column permutation of a CRS matrix, permutation of a vector, bandwidth (DESIGN.md "Reordering").
// EXTENSION: the reference has no permutation; the known answers are tests/reorder_model.py.
//
// A permutation is n u32 with perm[new] = old.  out[i][j] = a[row_perm[i]][col_perm[j]]: row i of the result is row
// row_perm[i] of a with the same entries in the same storage order, column c relabelled to col_perm^-1[c], values copied
// bit for bit; nothing is sorted.
//
//   k_perm_first / k_perm_check  validation, and the inverse as its by-product: first[p] = smallest i with perm[i] == p
//                                (integer atomicMin: independent of arrival order); position i is bad when perm[i] >= n or
//                                first[perm[i]] != i, and the smallest bad position is reported.  For a valid
//                                permutation first[] IS the inverse -- the scatter that builds col_perm^-1 once per call.
//   k_perm_row_lengths           len[i] = length of source row row_perm[i]; the library's scan turns them into offsets.
//   k_perm_tile_rows             the output row holding the first entry of every tile (one binary search per tile).
//   k_perm_emit                  parallel over OUTPUT entries: a workgroup takes kPermTile consecutive output entries, stages the
//                                offsets and source starts of the rows they lie in in LDS (tiles spanning more than
//                                kPermStageRows rows -- runs of empty rows -- search the offsets in memory instead), every thread
//                                writes 4 consecutive columns and values with 16-byte stores (fully coalesced) and reads
//                                them from its source rows, contiguous per row.  Addresses are 64-bit.
// Byte model of the emit pass, per entry: read 4 + sizeof(T) (source column and value), write 4 + sizeof(T), plus one
// 4-byte gather from col_perm^-1 when columns are permuted; per row 12 bytes of offsets.
#include "arg_stage.hpp"
#include "crs_forms.hpp"

namespace smh {

constexpr uint32_t kUnset = 0xFFFFFFFFu;
constexpr int kPermTile = 4 * kBlock;      // output entries per workgroup: 4 consecutive ones per thread
constexpr int kPermStageRows = 1024;       // rows of a tile whose offsets are staged in LDS

__global__ void __launch_bounds__(kBlock)
k_perm_first(const uint32_t *__restrict__ perm, uint64_t n, uint32_t *__restrict__ first) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t p = perm[i];
        if (p < n) atomicMin(&first[p], (uint32_t)i);
    }
}

__global__ void __launch_bounds__(kBlock)
k_perm_check(const uint32_t *__restrict__ perm, uint64_t n, const uint32_t *__restrict__ first, uint32_t *__restrict__ bad) {
    uint32_t mine = kUnset;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t p = perm[i];
        if ((p >= n || first[p] != (uint32_t)i) && (uint32_t)i < mine) mine = (uint32_t)i;
    }
    if (mine != kUnset) atomicMin(bad, mine);
}

// first [n]: scratch of the caller; afterwards the inverse of perm.  SMH_ERR_INVALID names the first offending position.
int validate_permutation(const uint32_t *perm, size_t n, uint32_t *first, const char *what, hipStream_t s) {
    if (n == 0) return SMH_OK;
    Scratch scr;
    uint32_t *d_bad = nullptr;
    SMH_TRY(scr.alloc(&d_bad, 1));
    SMH_HIP(hipMemsetAsync(first, 0xFF, n * sizeof(uint32_t), s));
    SMH_HIP(hipMemsetAsync(d_bad, 0xFF, sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_perm_first, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, perm, (uint64_t)n, first);
    SMH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_perm_check, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, perm, (uint64_t)n, first, d_bad);
    SMH_HIP(hipGetLastError());
    uint32_t bad = kUnset;
    SMH_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    SMH_HIP(hipStreamSynchronize(s));
    if (bad == kUnset) return SMH_OK;
    uint32_t p = 0;
    SMH_HIP(hipMemcpy(&p, perm + bad, sizeof p, hipMemcpyDeviceToHost));
    if ((size_t)p >= n) return fail(SMH_ERR_INVALID, "%s[%u] = %u is not below %zu", what, bad, p, n);
    return fail(SMH_ERR_INVALID, "%s[%u] = %u occurs twice", what, bad, p);
}

__global__ void __launch_bounds__(kBlock)
k_perm_row_lengths(const uint32_t *__restrict__ a_off, const uint32_t *__restrict__ row_perm, uint64_t n_rows, uint32_t *__restrict__ len) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_rows; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t l = 0;
        if (i < n_rows) {
            const uint64_t r = row_perm ? row_perm[i] : i;
            l = a_off[r + 1] - a_off[r];
        }
        len[i] = l;  // (len[n_rows] = 0: the scan leaves the total there)
    }
}

// the last row r in [lo, hi] with off[r] <= k (off[lo] <= k is the caller's)
__device__ __forceinline__ uint64_t last_row_at_or_below(const uint32_t *off, uint64_t lo, uint64_t hi, uint64_t k) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if ((uint64_t)off[mid] <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(kBlock)
k_perm_tile_rows(const uint32_t *__restrict__ out_off, uint64_t n_rows, uint64_t nnz, uint64_t n_tiles, uint32_t *__restrict__ tile_row) {
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= n_tiles; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = t * kPermTile;
        // (out_off[n_rows] = nnz: an entry index k < nnz lands in a row below n_rows)
        tile_row[t] = k < nnz ? (uint32_t)last_row_at_or_below(out_off, 0, n_rows - 1, k) : (uint32_t)(n_rows - 1);
    }
}

template <typename T> struct Vec4;
template <> struct Vec4<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct Vec4<double> { typedef double type __attribute__((ext_vector_type(4))); };

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_perm_emit(const uint32_t *__restrict__ a_off, const uint32_t *__restrict__ a_col, const T *__restrict__ a_val,
            const uint32_t *__restrict__ row_perm, const uint32_t *__restrict__ col_inv, const uint32_t *__restrict__ out_off,
            const uint32_t *__restrict__ tile_row, uint64_t nnz, uint32_t *__restrict__ out_col, T *__restrict__ out_val) {
    __shared__ uint32_t s_off[kPermStageRows + 1];  // offsets of the tile's rows (and of the one after them)
    __shared__ uint32_t s_src[kPermStageRows];      // where each of those rows starts in the source
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint64_t t = blockIdx.x;
    const uint64_t r0 = tile_row[t], r1 = tile_row[t + 1];  // rows of the tile's first entry and of the next tile's
    const uint64_t nr = r1 - r0 + 1;
    const bool staged = nr <= (uint64_t)kPermStageRows;
    if (staged) {
        for (uint64_t j = threadIdx.x; j <= nr; j += kBlock) s_off[j] = out_off[r0 + j];
        for (uint64_t j = threadIdx.x; j < nr; j += kBlock) s_src[j] = a_off[row_perm ? row_perm[r0 + j] : r0 + j];
        __syncthreads();
    }
    const uint64_t k0 = t * kPermTile + 4ull * threadIdx.x;
    if (k0 >= nnz) return;
    uint32_t c[4] = {0, 0, 0, 0};
    T v[4] = {T(0), T(0), T(0), T(0)};
    if (staged) {
        uint32_t lo = 0, hi = (uint32_t)nr - 1;  // last staged row whose offset is <= k0
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if ((uint64_t)s_off[mid] <= k0) lo = mid; else hi = mid - 1;
        }
        uint32_t j = lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint64_t k = k0 + e;
            if (k < nnz) {
                while ((uint64_t)s_off[j + 1] <= k) ++j;  // (ends: s_off[nr] > k for every entry of the tile, or k >= nnz)
                const uint64_t src = (uint64_t)s_src[j] + (k - s_off[j]);
                const uint32_t cc = a_col[src];
                c[e] = col_inv ? col_inv[cc] : cc;
                v[e] = a_val[src];
            }
        }
    } else {
        uint64_t r = last_row_at_or_below(out_off, r0, r1, k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint64_t k = k0 + e;
            if (k < nnz) {
                while ((uint64_t)out_off[r + 1] <= k) ++r;
                const uint64_t src = (uint64_t)a_off[row_perm ? row_perm[r] : r] + (k - out_off[r]);
                const uint32_t cc = a_col[src];
                c[e] = col_inv ? col_inv[cc] : cc;
                v[e] = a_val[src];
            }
        }
    }
    // 16-byte stores: k0 is a multiple of 4, the arrays are padded by 4 entries (written as zeros here)
    u32x4 cv;
    cv.x = c[0]; cv.y = c[1]; cv.z = c[2]; cv.w = c[3];
    *reinterpret_cast<u32x4 *>(out_col + k0) = cv;
    typename Vec4<T>::type vv;
    vv.x = v[0]; vv.y = v[1]; vv.z = v[2]; vv.w = v[3];
    *reinterpret_cast<typename Vec4<T>::type *>(out_val + k0) = vv;
}

// The arrays of the permuted matrix.  row_perm / col_inv: device arrays or null (identity); col_inv is the INVERSE of the column
// permutation.  a with at least one row; every column of a below the length of col_inv (the caller's checks).
int permute_crs(int dtype, const uint32_t *a_off, const uint32_t *a_col, const void *a_val, size_t n_rows, size_t nnz, const uint32_t *row_perm,
                const uint32_t *col_inv, CrsArrays *out, hipStream_t s) {
    const size_t vs = dtype_size(dtype);
    SMH_TRY(out->alloc_off(n_rows));
    hipLaunchKernelGGL(k_perm_row_lengths, dim3(grid_for(n_rows + 1, kBuildGrid)), dim3(kBlock), 0, s, a_off, row_perm, (uint64_t)n_rows, out->off);
    SMH_HIP(hipGetLastError());
    uint64_t total = 0;
    SMH_TRY(device_exclusive_scan_u32(out->off, n_rows + 1, s, &total));
    if (total != nnz) return fail(SMH_ERR_INVALID, "permuted rows hold %llu entries, the matrix %zu", (unsigned long long)total, nnz);
    SMH_TRY(out->alloc_entries(nnz, vs));
    SMH_TRY(out->zero_padding(nnz, vs, s));
    if (nnz == 0) {
        SMH_HIP(hipStreamSynchronize(s));
        return SMH_OK;
    }
    const uint64_t n_tiles = ((uint64_t)nnz + kPermTile - 1) / kPermTile;
    Scratch scr;
    uint32_t *d_tile_row = nullptr;
    SMH_TRY(scr.alloc(&d_tile_row, n_tiles + 1));
    hipLaunchKernelGGL(k_perm_tile_rows, dim3(grid_for(n_tiles + 1, kBuildGrid)), dim3(kBlock), 0, s, out->off, (uint64_t)n_rows, (uint64_t)nnz, n_tiles,
                       d_tile_row);
    SMH_HIP(hipGetLastError());
    if (dtype == SMH_F64)
        hipLaunchKernelGGL(k_perm_emit<double>, dim3((unsigned)n_tiles), dim3(kBlock), 0, s, a_off, a_col, (const double *)a_val, row_perm, col_inv,
                           out->off, d_tile_row, (uint64_t)nnz, out->col, (double *)out->val);
    else
        hipLaunchKernelGGL(k_perm_emit<float>, dim3((unsigned)n_tiles), dim3(kBlock), 0, s, a_off, a_col, (const float *)a_val, row_perm, col_inv, out->off,
                           d_tile_row, (uint64_t)nnz, out->col, (float *)out->val);
    SMH_HIP(hipGetLastError());
    SMH_HIP(hipStreamSynchronize(s));
    return SMH_OK;
}

// ---- vectors: gather dst[i] = src[perm[i]], scatter dst[perm[i]] = src[i] ----------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_vec_permute(T *__restrict__ dst, const T *__restrict__ src, const uint32_t *__restrict__ perm, uint64_t n, int inverse) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = perm[i];
        if (inverse) dst[p] = src[i]; else dst[i] = src[p];
    }
}

int launch_vec_permute(int dtype, void *dst, const void *src, const uint32_t *perm, size_t n, bool inverse, hipStream_t s) {
    if (n == 0) return SMH_OK;
    if (dtype == SMH_F64)
        hipLaunchKernelGGL(k_vec_permute<double>, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, (double *)dst, (const double *)src, perm, (uint64_t)n,
                           inverse ? 1 : 0);
    else
        hipLaunchKernelGGL(k_vec_permute<float>, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, (float *)dst, (const float *)src, perm, (uint64_t)n,
                           inverse ? 1 : 0);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// ---- bandwidth: one pass, integer max -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_bandwidth(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, uint64_t n_rows, uint32_t *__restrict__ out2) {
    uint32_t lower = 0, upper = 0;  // max i - j, max j - i
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t e1 = off[i + 1];
        for (uint64_t e = off[i]; e < e1; ++e) {
            const uint64_t j = col[e];
            if (i > j && (uint32_t)(i - j) > lower) lower = (uint32_t)(i - j);
            if (j > i && (uint32_t)(j - i) > upper) upper = (uint32_t)(j - i);
        }
    }
    lower = wave_max_u32(lower);
    upper = wave_max_u32(upper);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (lower) atomicMax(&out2[0], lower);
        if (upper) atomicMax(&out2[1], upper);
    }
}

int launch_bandwidth(const uint32_t *off, const uint32_t *col, size_t n_rows, uint32_t *d_out2, hipStream_t s) {
    SMH_HIP(hipMemsetAsync(d_out2, 0, 2 * sizeof(uint32_t), s));
    if (n_rows == 0) return SMH_OK;
    hipLaunchKernelGGL(k_bandwidth, dim3(grid_for(n_rows, kBuildGrid)), dim3(kBlock), 0, s, off, col, (uint64_t)n_rows, d_out2);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// ---- the entry points: a permutation is n u32 with perm[new] = old (EXTENSION) ---------------------------------------------------
// One permutation argument of an entry point: checked for its length, staged (a host array goes to the device, the caller's
// device array is checked), validated there (`inv` = its inverse afterwards).  perm == NULL: the identity, nothing to do
// (*d_perm stays null).
static int take_permutation(ArgStage &st, const uint32_t *perm, size_t len, size_t n, const char *what, const uint32_t **d_perm, uint32_t **inv) {
    *d_perm = nullptr;
    *inv = nullptr;
    if (!perm) return SMH_OK;
    if (len != n) return fail(SMH_ERR_DIM_MISMATCH, "%s has %zu entries, %zu expected", what, len, n);
    if (n == 0) return SMH_OK;
    const void *d = nullptr;
    SMH_TRY(st.in(perm, n * sizeof(uint32_t), what, &d));
    *d_perm = (const uint32_t *)d;
    SMH_TRY(st.scratch().alloc(inv, n));
    return validate_permutation(*d_perm, n, *inv, what, nullptr);
}

static int permute_common(const smh_crs *a, const uint32_t *row_perm, size_t n_row_perm, const uint32_t *col_perm, size_t n_col_perm, bool on_device,
                          smh_crs **out) {
    if (!out) return fail(SMH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!a) return fail(SMH_ERR_INVALID, "NULL handle");
    if (a->orphans) return fail(SMH_ERR_INVALID, "a handle holding an orphaned entry cannot be permuted");
    if (col_perm) SMH_TRY(columns_within_n_cols(a, "permute"));
    ArgStage st(on_device, a->device);
    SMH_TRY(st.callers_writes_first());  // known difference, kept: before the device check (take_permutation)
    SMH_HIP(hipStreamSynchronize(a->stream));
    const uint32_t *d_rp = nullptr, *d_cp = nullptr;
    uint32_t *row_inv = nullptr, *col_inv = nullptr;
    SMH_TRY(take_permutation(st, row_perm, n_row_perm, a->n_rows, "row_perm", &d_rp, &row_inv));
    SMH_TRY(take_permutation(st, col_perm, n_col_perm, a->n_cols, "col_perm", &d_cp, &col_inv));
    CrsArrays arrays;
    SMH_TRY(permute_crs(a->dtype, a->d_off, a->d_col, a->d_val, a->n_rows, a->nnz, d_rp, col_inv, &arrays, nullptr));
    return wrap_arrays(a->dtype, a, a->n_rows, a->n_cols, a->nnz, arrays, 0, out);
}

static int permute_symmetric_common(const smh_crs *a, const uint32_t *perm, size_t n_perm, bool on_device, smh_crs **out) {
    if (!out) return fail(SMH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!a || !perm) return fail(SMH_ERR_INVALID, "NULL argument");
    if (a->n_rows != a->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    if (a->orphans) return fail(SMH_ERR_INVALID, "a handle holding an orphaned entry cannot be permuted");
    SMH_TRY(columns_within_n_cols(a, "permute_symmetric"));
    ArgStage st(on_device, a->device);
    SMH_TRY(st.callers_writes_first());  // known difference, kept: before the device check (take_permutation)
    SMH_HIP(hipStreamSynchronize(a->stream));
    const uint32_t *d_p = nullptr;
    uint32_t *inv = nullptr;
    SMH_TRY(take_permutation(st, perm, n_perm, a->n_rows, "perm", &d_p, &inv));  // (validated once, one inverse)
    CrsArrays arrays;
    SMH_TRY(permute_crs(a->dtype, a->d_off, a->d_col, a->d_val, a->n_rows, a->nnz, d_p, inv, &arrays, nullptr));
    return wrap_arrays(a->dtype, a, a->n_rows, a->n_cols, a->nnz, arrays, 0, out);
}

static int vec_permute_common(smh_vec *dst, const smh_vec *src, const uint32_t *perm, size_t n_perm, int inverse, bool on_device) {
    SMH_TRY(vec_check_pair(dst, src));
    if (!perm && n_perm) return fail(SMH_ERR_INVALID, "perm is NULL");
    if (dst->n != src->n) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    if (dst == src || (dst->d && dst->d == src->d)) return fail(SMH_ERR_INVALID, "a vector cannot be permuted into itself");
    if (n_perm != src->n) return fail(SMH_ERR_DIM_MISMATCH, "perm has %zu entries, %zu expected", n_perm, src->n);
    if (src->n == 0) return SMH_OK;
    // known difference, kept: device-wide in BOTH forms (vectors work on the null stream; the caller's writes to a device array come first)
    SMH_HIP(hipDeviceSynchronize());
    ArgStage st(on_device, src->device);
    const uint32_t *d_p = nullptr;
    uint32_t *inv = nullptr;
    SMH_TRY(take_permutation(st, perm, n_perm, src->n, "perm", &d_p, &inv));
    SMH_TRY(launch_vec_permute(src->dtype, dst->d, src->d, d_p, src->n, inverse != 0, nullptr));
    SMH_HIP(hipStreamSynchronize(nullptr));
    return SMH_OK;
}

}  // namespace smh

using namespace smh;

extern "C" {

int smh_crs_permute(const smh_crs *a, const uint32_t *row_perm, size_t n_row_perm, const uint32_t *col_perm, size_t n_col_perm, smh_crs **out) {
    return permute_common(a, row_perm, n_row_perm, col_perm, n_col_perm, false, out);
}
int smh_crs_permute_dev(const smh_crs *a, const uint32_t *row_perm_dev, size_t n_row_perm, const uint32_t *col_perm_dev, size_t n_col_perm,
                        smh_crs **out) {
    return permute_common(a, row_perm_dev, n_row_perm, col_perm_dev, n_col_perm, true, out);
}

int smh_crs_permute_symmetric(const smh_crs *a, const uint32_t *perm, size_t n_perm, smh_crs **out) {
    return permute_symmetric_common(a, perm, n_perm, false, out);
}
int smh_crs_permute_symmetric_dev(const smh_crs *a, const uint32_t *perm_dev, size_t n_perm, smh_crs **out) {
    return permute_symmetric_common(a, perm_dev, n_perm, true, out);
}

int smh_vec_permute(smh_vec *dst, const smh_vec *src, const uint32_t *perm, size_t n_perm, int inverse) {
    return vec_permute_common(dst, src, perm, n_perm, inverse, false);
}
int smh_vec_permute_dev(smh_vec *dst, const smh_vec *src, const uint32_t *perm_dev, size_t n_perm, int inverse) {
    return vec_permute_common(dst, src, perm_dev, n_perm, inverse, true);
}

}  // extern "C"
