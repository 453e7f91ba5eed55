// mvec.hip -- smh_mvec: k DenseVecs of one dimension held against one matrix (load cases, block Krylov methods, subspace
// iteration), and the entry points of the multi-vector product K1m (spmv_many.hip).
//
// Layout: INTERLEAVED -- element i of vector c at d[i * ld + c], ld = k rounded up to a multiple of 4, padding columns zero.  The
// product's gather of x[col] for four vectors is then one aligned 16-byte load (f32; two in f64) and a row of the result one
// 16-byte store.  The host format is what k DenseVecs look like: k vectors of n entries, one after the other.  Both
// transpositions run on the device: the host format goes through a staging array and a kernel that turns 64 x 32 tiles in LDS
// (coalesced on both sides); a column is exchanged with a DenseVec by 16-byte read-modify-writes of the row groups that hold it
// (no 4-byte strided stores).  Host-side logic otherwise: statuses are decided before anything is launched.
#include <new>

#include "internal.hpp"

namespace smh {

static bool mv_valid_dtype(int dt) { return dt == SMH_F32 || dt == SMH_F64; }

constexpr int kMvTileRows = 64, kMvTileCols = 32;

// host format (src: k vectors of n) -> interleaved (dst: n rows of ld); columns k .. ld - 1 are written as +0
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_mvec_pack(const T *__restrict__ src, T *__restrict__ dst, uint64_t n, uint32_t k, uint32_t ld, uint64_t n_tiles) {
    __shared__ T s[kMvTileCols][kMvTileRows + 1];
    const uint32_t t = threadIdx.x;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i0 = tile * kMvTileRows;
        for (uint32_t cb = 0; cb < ld; cb += kMvTileCols) {
            const uint32_t w = ld - cb < (uint32_t)kMvTileCols ? ld - cb : (uint32_t)kMvTileCols;
            // in: a run of 64 entries of one vector per wavefront
            for (uint32_t cc = t / kMvTileRows; cc < w; cc += kBlock / kMvTileRows) {
                const uint32_t ii = t % kMvTileRows;
                const uint64_t i = i0 + ii;
                s[cc][ii] = (cb + cc < k && i < n) ? src[(uint64_t)(cb + cc) * n + i] : T(0);
            }
            __syncthreads();
            // out: the tile's 64 rows of w columns in address order (one contiguous run when w == ld)
            for (uint32_t e = t; e < (uint32_t)kMvTileRows * w; e += kBlock) {
                const uint32_t ii = e / w, cc = e % w;
                if (i0 + ii < n) dst[(i0 + ii) * ld + cb + cc] = s[cc][ii];
            }
            __syncthreads();
        }
    }
}

// interleaved (src: n rows of ld) -> host format (dst: k vectors of n)
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_mvec_unpack(const T *__restrict__ src, T *__restrict__ dst, uint64_t n, uint32_t k, uint32_t ld, uint64_t n_tiles) {
    __shared__ T s[kMvTileCols][kMvTileRows + 1];
    const uint32_t t = threadIdx.x;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i0 = tile * kMvTileRows;
        for (uint32_t cb = 0; cb < k; cb += kMvTileCols) {
            const uint32_t w = ld - cb < (uint32_t)kMvTileCols ? ld - cb : (uint32_t)kMvTileCols;
            for (uint32_t e = t; e < (uint32_t)kMvTileRows * w; e += kBlock) {
                const uint32_t ii = e / w, cc = e % w;
                s[cc][ii] = i0 + ii < n ? src[(i0 + ii) * ld + cb + cc] : T(0);
            }
            __syncthreads();
            for (uint32_t cc = t / kMvTileRows; cc < w; cc += kBlock / kMvTileRows) {
                const uint32_t ii = t % kMvTileRows;
                const uint64_t i = i0 + ii;
                if (cb + cc < k && i < n) dst[(uint64_t)(cb + cc) * n + i] = s[cc][ii];
            }
            __syncthreads();
        }
    }
}

// column c <-> a DenseVec: one 16-byte group of row i (4 f32 / 2 f64 columns) per thread
template <typename T, bool SET>
__global__ void __launch_bounds__(kBlock)
k_mvec_column(T *__restrict__ d, T *__restrict__ v, uint64_t n, uint64_t ld, uint32_t c) {
    constexpr uint32_t G = 16 / sizeof(T);
    typedef T group_t __attribute__((ext_vector_type(G)));
    const uint32_t cg = c & ~(G - 1), e = c & (G - 1);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        group_t *p = reinterpret_cast<group_t *>(d + i * ld + cg);
        group_t g = *p;
        if constexpr (SET) {
            g[e] = v[i];
            *p = g;
        } else {
            v[i] = g[e];
        }
    }
}

static int mv_transpose(int dtype, bool pack, const void *src, void *dst, size_t n, size_t k, size_t ld, hipStream_t s) {
    if (n == 0) return SMH_OK;
    const uint64_t n_tiles = (n + kMvTileRows - 1) / kMvTileRows;
    const dim3 grid((unsigned)(n_tiles < kBuildGrid ? n_tiles : kBuildGrid)), block(kBlock);
    if (dtype == SMH_F64) {
        if (pack) hipLaunchKernelGGL(k_mvec_pack<double>, grid, block, 0, s, (const double *)src, (double *)dst, (uint64_t)n, (uint32_t)k, (uint32_t)ld, n_tiles);
        else hipLaunchKernelGGL(k_mvec_unpack<double>, grid, block, 0, s, (const double *)src, (double *)dst, (uint64_t)n, (uint32_t)k, (uint32_t)ld, n_tiles);
    } else {
        if (pack) hipLaunchKernelGGL(k_mvec_pack<float>, grid, block, 0, s, (const float *)src, (float *)dst, (uint64_t)n, (uint32_t)k, (uint32_t)ld, n_tiles);
        else hipLaunchKernelGGL(k_mvec_unpack<float>, grid, block, 0, s, (const float *)src, (float *)dst, (uint64_t)n, (uint32_t)k, (uint32_t)ld, n_tiles);
    }
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

static int mv_column(int dtype, bool set, void *d, void *v, size_t n, size_t ld, size_t c, hipStream_t s) {
    if (n == 0) return SMH_OK;
    const dim3 grid(grid_for(n, kBuildGrid)), block(kBlock);
    if (dtype == SMH_F64) {
        if (set) hipLaunchKernelGGL((k_mvec_column<double, true>), grid, block, 0, s, (double *)d, (double *)v, (uint64_t)n, (uint64_t)ld, (uint32_t)c);
        else hipLaunchKernelGGL((k_mvec_column<double, false>), grid, block, 0, s, (double *)d, (double *)v, (uint64_t)n, (uint64_t)ld, (uint32_t)c);
    } else {
        if (set) hipLaunchKernelGGL((k_mvec_column<float, true>), grid, block, 0, s, (float *)d, (float *)v, (uint64_t)n, (uint64_t)ld, (uint32_t)c);
        else hipLaunchKernelGGL((k_mvec_column<float, false>), grid, block, 0, s, (float *)d, (float *)v, (uint64_t)n, (uint64_t)ld, (uint32_t)c);
    }
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// ld and the storage size of k vectors of n entries; SMH_ERR_INVALID for k == 0, a bad dtype or n * ld * sizeof(T) overflowing
static int mv_geometry(int dtype, size_t n, size_t k, size_t *ld_out, size_t *bytes_out) {
    if (!mv_valid_dtype(dtype)) return fail(SMH_ERR_INVALID, "dtype must be SMH_F32 or SMH_F64");
    if (k == 0) return fail(SMH_ERR_INVALID, "a multi-vector holds at least one vector (k == 0)");
    if (k > 0xFFFFFFFCull) return fail(SMH_ERR_INVALID, "the vector count %zu does not fit the u32 index type", k);
    const size_t ld = (k + 3) & ~(size_t)3;
    size_t elems = 0, bytes = 0;
    if (__builtin_mul_overflow(n, ld, &elems) || __builtin_mul_overflow(elems, dtype_size(dtype), &bytes))
        return fail(SMH_ERR_INVALID, "a multi-vector of %zu x %zu entries does not fit the address space", n, ld);
    *ld_out = ld;
    *bytes_out = bytes;
    return SMH_OK;
}

// fills *mv (empty) with zeroed storage; the zero fill is enqueued on s
static int mv_alloc(smh_mvec *mv, int dtype, size_t n, size_t k, hipStream_t s) {
    size_t ld = 0, bytes = 0;
    SMH_TRY(mv_geometry(dtype, n, k, &ld, &bytes));
    SMH_TRY(mv->d.alloc(bytes ? bytes : 16));
    SMH_HIP(hipMemsetAsync(mv->d.get(), 0, bytes ? bytes : 16, s));
    mv->dtype = dtype; mv->device = current_device(); mv->n = n; mv->k = k; mv->ld = ld;
    return SMH_OK;
}

// host format <-> mv through a device staging array; synchronises s
static int mv_copy_host(const smh_mvec *mv, const void *host_in, void *host_out, hipStream_t s) {
    const size_t bytes = mv->n * mv->k * dtype_size(mv->dtype);
    if (bytes == 0) return SMH_OK;
    Scratch scr;
    char *stage = nullptr;
    SMH_TRY(scr.alloc(&stage, bytes));
    if (host_in) {
        SMH_HIP(hipMemcpyAsync(stage, host_in, bytes, hipMemcpyHostToDevice, s));
        SMH_TRY(mv_transpose(mv->dtype, true, stage, mv->d.get(), mv->n, mv->k, mv->ld, s));
    } else {
        SMH_TRY(mv_transpose(mv->dtype, false, mv->d.get(), stage, mv->n, mv->k, mv->ld, s));
        SMH_HIP(hipMemcpyAsync(host_out, stage, bytes, hipMemcpyDeviceToHost, s));
    }
    SMH_HIP(hipStreamSynchronize(s));  // (before the staging array returns to the pool)
    return SMH_OK;
}

// every status of the product, decided before any launch; then the sweeps are enqueued on s (nothing allocated, nothing awaited)
static int many_enqueue(smh_crs *m, const void *x, size_t x_len, void *y, size_t k, size_t ld, hipStream_t s) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (k == 0) return fail(SMH_ERR_INVALID, "a multi-vector holds at least one vector (k == 0)");
    if (ld < k || ld % 4 != 0 || ld > 0xFFFFFFFCull) return fail(SMH_ERR_INVALID, "ld must be a multiple of 4 and at least k (k = %zu, ld = %zu)", k, ld);
    const size_t vs = dtype_size(m->dtype);
    size_t t = 0;
    if (__builtin_mul_overflow(x_len, ld, &t) || __builtin_mul_overflow(t, vs, &t) || __builtin_mul_overflow(m->n_rows, ld, &t) ||
        __builtin_mul_overflow(t, vs, &t))
        return fail(SMH_ERR_INVALID, "a multi-vector of %zu x %zu entries does not fit the address space", x_len > m->n_rows ? x_len : m->n_rows, ld);
    if (m->n_rows && (!y || (m->nnz && !x))) return fail(SMH_ERR_INVALID, "NULL device vector");
    if (x && x == y) return fail(SMH_ERR_INVALID, "x and y are the same storage: the product cannot run in place");
    if (((uintptr_t)x | (uintptr_t)y) & 15u) return fail(SMH_ERR_INVALID, "multi-vector storage must be 16-byte aligned");
    if (m->nnz > 0 && (size_t)m->max_col >= x_len)
        return fail(SMH_ERR_INDEX_RANGE, "index out of bounds: the len is %zu but the index is %u", x_len, m->max_col);
    return launch_spmv_many(m->dtype, m->d_off, m->d_col, m->d_val, x, y, m->n_rows, m->nnz, m->owns, k, ld, s);
}

}  // namespace smh

using namespace smh;

extern "C" {

int smh_mvec_create(smh_dtype dtype, size_t n, size_t k, smh_mvec **out) {
    if (!out) return fail(SMH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    size_t ld = 0, bytes = 0;
    SMH_TRY(mv_geometry(dtype, n, k, &ld, &bytes));
    SMH_TRY(require_device());
    smh_mvec *mv = new (std::nothrow) smh_mvec();
    if (!mv) return fail(SMH_ERR_OOM, "host allocation failed");
    int rc = mv_alloc(mv, dtype, n, k, nullptr);
    if (rc == SMH_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = hip_fail(hipGetLastError(), "smh_mvec_create", __FILE__, __LINE__);
    if (rc != SMH_OK) { delete mv; return rc; }
    *out = mv;
    return SMH_OK;
}

int smh_mvec_from_host(smh_dtype dtype, size_t n, size_t k, const void *host, smh_mvec **out) {
    SMH_TRY(smh_mvec_create(dtype, n, k, out));
    if (n) {
        const int rc = smh_mvec_upload(*out, host);
        if (rc != SMH_OK) return keep_error(rc, [&] { smh_mvec_destroy(*out); *out = nullptr; });
    }
    return SMH_OK;
}

int smh_mvec_destroy(smh_mvec *mv) {
    delete mv;  // (the storage goes back to the pool with it)
    return SMH_OK;
}

int smh_mvec_upload(smh_mvec *mv, const void *host) {
    if (!mv || (mv->n && !host)) return fail(SMH_ERR_INVALID, "NULL argument");
    return mv_copy_host(mv, host, nullptr, nullptr);
}

int smh_mvec_download(const smh_mvec *mv, void *host) {
    if (!mv || (mv->n && !host)) return fail(SMH_ERR_INVALID, "NULL argument");
    return mv_copy_host(mv, nullptr, host, nullptr);
}

size_t smh_mvec_dim(const smh_mvec *mv) { return mv ? mv->n : 0; }
size_t smh_mvec_count(const smh_mvec *mv) { return mv ? mv->k : 0; }
size_t smh_mvec_ld(const smh_mvec *mv) { return mv ? mv->ld : 0; }
int smh_mvec_dtype(const smh_mvec *mv) { return mv ? mv->dtype : -1; }
void *smh_mvec_data(const smh_mvec *mv) { return mv ? (void *)mv->d.get() : nullptr; }

static int column_args(const smh_mvec *mv, size_t c, const smh_vec *v) {
    if (!mv || !v) return fail(SMH_ERR_INVALID, "NULL argument");
    if (c >= mv->k) return fail(SMH_ERR_INVALID, "column %zu of a multi-vector of %zu vectors", c, mv->k);
    if (v->dtype != mv->dtype) return fail(SMH_ERR_INVALID, "vector dtype mismatch");
    if (v->n != mv->n) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    return SMH_OK;
}

int smh_mvec_set_column(smh_mvec *mv, size_t c, const smh_vec *v) {
    SMH_TRY(column_args(mv, c, v));
    SMH_TRY(mv_column(mv->dtype, true, mv->d.get(), v->d, mv->n, mv->ld, c, nullptr));
    SMH_HIP(hipStreamSynchronize(nullptr));
    return SMH_OK;
}

int smh_mvec_get_column(const smh_mvec *mv, size_t c, smh_vec *v) {
    SMH_TRY(column_args(mv, c, v));
    SMH_TRY(mv_column(mv->dtype, false, mv->d.get(), v->d, mv->n, mv->ld, c, nullptr));
    SMH_HIP(hipStreamSynchronize(nullptr));
    return SMH_OK;
}

int smh_crs_spmv_many(smh_crs *m, const smh_mvec *x, smh_mvec *y) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (!x || !y) return fail(SMH_ERR_INVALID, "NULL multi-vector handle");
    if (x->dtype != m->dtype || y->dtype != m->dtype) return fail(SMH_ERR_INVALID, "multi-vector dtype differs from the matrix's");
    if (x == y) return fail(SMH_ERR_INVALID, "x and y are the same storage: the product cannot run in place");
    if (y->n != m->n_rows || y->k != x->k) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    SMH_TRY(many_enqueue(m, x->d.get(), x->n, y->d.get(), x->k, x->ld, m->stream));
    SMH_HIP(hipStreamSynchronize(m->stream));
    return SMH_OK;
}

int smh_crs_spmv_many_dev(smh_crs *m, const void *x_dev, size_t x_len, void *y_dev, size_t k, size_t ld, void *stream) {
    return many_enqueue(m, x_dev, x_len, y_dev, k, ld, (hipStream_t)stream);
}

int smh_crs_spmv_many_host(smh_crs *m, const void *x_host, size_t x_len, size_t k, void *y_host) {
    if (k == 0) return fail(SMH_ERR_INVALID, "a multi-vector holds at least one vector (k == 0)");
    SMH_TRY(require_device());
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if ((m->n_rows && !y_host) || (x_len && !x_host)) return fail(SMH_ERR_INVALID, "NULL host vector");
    if (m->nnz > 0 && (size_t)m->max_col >= x_len)
        return fail(SMH_ERR_INDEX_RANGE, "index out of bounds: the len is %zu but the index is %u", x_len, m->max_col);
    if (m->n_rows == 0) return SMH_OK;
    smh_mvec x, y;  // (their storage goes back to the pool at the end of this call)
    SMH_TRY(mv_alloc(&x, m->dtype, x_len, k, m->stream));
    SMH_TRY(mv_alloc(&y, m->dtype, m->n_rows, k, m->stream));
    SMH_TRY(mv_copy_host(&x, x_host, nullptr, m->stream));
    SMH_TRY(many_enqueue(m, x.d.get(), x_len, y.d.get(), k, x.ld, m->stream));
    return mv_copy_host(&y, nullptr, y_host, m->stream);
}

}  // extern "C"
