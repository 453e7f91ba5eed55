// mvec_blas.hip -- the per-column BLAS-1 of smh_mvec (densevec.rs:51-73 and vector.rs:50-58, k times) and the column tree
// that it shares with the k-column solver (cg_many.hip).
//
// Element-wise operations run over the interleaved storage as it lies: one 16-byte ROW GROUP (4 f32 / 2 f64 columns of one row)
// per load and store, non-temporal, every operation one explicit *_rn rounding.  add / sub keep the padding columns at +0
// because +0 +- +0 is +0; scale SELECTS: a column at or beyond k is stored back as it was read, so an infinite or NaN factor
// cannot turn a padding zero into NaN.
//
// The column tree: column c is summed in an order that depends on n alone -- not on k, ld, c or the
// other columns.  With B = min(reduce_blocks(n), cap) workgroups of 256 threads per row group (cap 512, the single solver's), thread
// g = 256 w + t starts from T(0) and adds the rounded terms of rows g, g + 256 B, ... in that order; a wavefront folds by
// __shfl_down (32, 16, ..., 1); thread 0 adds the four wave sums in order from T(0): partial[c * B + w].  One 256-thread fold
// over the B partials of a column follows: thread t adds partial[t], then partial[t + 256], from T(0), then the same
// workgroup sum.  The grid is (row groups, B): blockIdx.x names the group so that the workgroups that share a cache line of a
// row (ld > one group) are dispatched next to each other.
#include "mvec_tree.hpp"

namespace smh {

enum class MvEw { Add, Sub, RSubInto };

// x = x + y / x - y / y - x over the whole storage (nv row groups); y may be x
template <typename T, MvEw OP>
__global__ void __launch_bounds__(kBlock) k_mvec_ew(T *x, const T *y, uint64_t nv) {
    typedef typename MvGroup<T>::type V;
    constexpr int G = MvGroup<T>::N;
    V *xv = reinterpret_cast<V *>(x);
    const V *yv = reinterpret_cast<const V *>(y);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nv; i += (uint64_t)gridDim.x * kBlock) {
        V a = __builtin_nontemporal_load(xv + i);
        const V b = __builtin_nontemporal_load(yv + i);
#pragma unroll
        for (int e = 0; e < G; ++e) {
            if constexpr (OP == MvEw::Add) a[e] = mv_add(a[e], b[e]);        // densevec.rs:51-58
            else if constexpr (OP == MvEw::Sub) a[e] = mv_sub(a[e], b[e]);   // :60-67
            else a[e] = mv_sub(b[e], a[e]);                                  // r = b - A x  (linearsolver.rs:38)
        }
        __builtin_nontemporal_store(a, xv + i);
    }
}

// x_c *= fac[c] for c < k (:69-73); fac: ld factors of T
template <typename T>
__global__ void __launch_bounds__(kBlock) k_mvec_scale(T *__restrict__ x, const T *__restrict__ fac, uint64_t nv, uint32_t ngroups, uint32_t k) {
    typedef typename MvGroup<T>::type V;
    constexpr int G = MvGroup<T>::N;
    V *xv = reinterpret_cast<V *>(x);
    const V *fv = reinterpret_cast<const V *>(fac);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nv; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t grp = (uint32_t)(i % ngroups);
        V a = __builtin_nontemporal_load(xv + i);
        const V f = fv[grp];
#pragma unroll
        for (int e = 0; e < G; ++e) {
            const T t = mv_mul(a[e], f[e]);
            a[e] = grp * G + e < k ? t : a[e];
        }
        __builtin_nontemporal_store(a, xv + i);
    }
}

// partials[c * gridDim.y + blockIdx.y] = this workgroup's share of x_c . y_c, for the columns of the row groups blockIdx.x, + gridDim.x, ...
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_mvec_dot(const T *__restrict__ x, const T *__restrict__ y, uint64_t n, uint32_t ngroups, T *__restrict__ partials) {
    typedef typename MvGroup<T>::type V;
    constexpr int G = MvGroup<T>::N;
    __shared__ T s_w[G][kBlock / kWave];
    __shared__ T s_sum[G];
    const V *xv = reinterpret_cast<const V *>(x);
    const V *yv = reinterpret_cast<const V *>(y);
    const uint64_t stride = (uint64_t)gridDim.y * kBlock;
    for (uint32_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        T acc[G];
#pragma unroll
        for (int e = 0; e < G; ++e) acc[e] = T(0);
        for (uint64_t i = (uint64_t)blockIdx.y * kBlock + threadIdx.x; i < n; i += stride) {
            const V a = __builtin_nontemporal_load(xv + i * ngroups + grp);
            const V b = __builtin_nontemporal_load(yv + i * ngroups + grp);
#pragma unroll
            for (int e = 0; e < G; ++e) acc[e] += mv_mul(a[e], b[e]);
        }
        mv_block_sums<T, G>(acc, s_w, s_sum);
        if (threadIdx.x < G) partials[(uint64_t)(grp * G + threadIdx.x) * gridDim.y + blockIdx.y] = s_sum[threadIdx.x];
        __syncthreads();  // (s_sum is read before the next group's sums arrive)
    }
}

// out[c] = fold of the nb partials of column c: one workgroup per column
template <typename T>
__global__ void __launch_bounds__(kBlock) k_mvec_fold(const T *__restrict__ partials, uint32_t nb, uint32_t ld, T *__restrict__ out) {
    __shared__ T s_w[1][kBlock / kWave];
    __shared__ T s_sum[1];
    for (uint32_t c = blockIdx.x; c < ld; c += gridDim.x) {
        T acc[1] = {T(0)};
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) acc[0] += partials[(uint64_t)c * nb + i];
        mv_block_sums<T, 1>(acc, s_w, s_sum);
        if (threadIdx.x == 0) out[c] = s_sum[0];
        __syncthreads();
    }
}

unsigned reduce_blocks(size_t n);  // blas1.hip

unsigned mv_tree_blocks(size_t n) {
    // the single solver's cap and its tuning knob (cg.hip): two workgroups per CU
    static const unsigned cap = getenv("SMH_CG_BLOCKS") && atoi(getenv("SMH_CG_BLOCKS")) > 0 ? (unsigned)atoi(getenv("SMH_CG_BLOCKS")) : 512u;
    const unsigned rb = reduce_blocks(n);
    return rb < cap ? rb : cap;
}

static inline unsigned mv_group_grid(size_t ngroups) { return (unsigned)(ngroups < 1024 ? ngroups : 1024); }

template <typename T>
static int mv_dot_partials_t(const void *x, const void *y, size_t n, size_t ld, void *partials, unsigned *nb_out, hipStream_t s) {
    const unsigned nb = mv_tree_blocks(n);
    const size_t ngroups = ld / MvGroup<T>::N;
    hipLaunchKernelGGL(k_mvec_dot<T>, dim3(mv_group_grid(ngroups), nb), dim3(kBlock), 0, s, (const T *)x, (const T *)y, (uint64_t)n, (uint32_t)ngroups,
                       (T *)partials);
    SMH_HIP(hipGetLastError());
    *nb_out = nb;
    return SMH_OK;
}

int mv_dot_partials(int dtype, const void *x, const void *y, size_t n, size_t ld, void *partials, unsigned *nb_out, hipStream_t s) {
    if (dtype == SMH_F64) return mv_dot_partials_t<double>(x, y, n, ld, partials, nb_out, s);
    return mv_dot_partials_t<float>(x, y, n, ld, partials, nb_out, s);
}

int mv_rsub_into(int dtype, void *r, const void *b, size_t n, size_t ld, hipStream_t s) {
    const uint64_t nv = (uint64_t)n * ld * dtype_size(dtype) / 16;
    if (nv == 0) return SMH_OK;
    const dim3 grid(grid_for(nv, kBuildGrid)), block(kBlock);
    if (dtype == SMH_F64) hipLaunchKernelGGL((k_mvec_ew<double, MvEw::RSubInto>), grid, block, 0, s, (double *)r, (const double *)b, nv);
    else hipLaunchKernelGGL((k_mvec_ew<float, MvEw::RSubInto>), grid, block, 0, s, (float *)r, (const float *)b, nv);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

static int mv_addsub(smh_mvec *x, const smh_mvec *y, bool sub) {
    const uint64_t nv = (uint64_t)x->n * x->ld * dtype_size(x->dtype) / 16;
    if (nv == 0) return SMH_OK;
    const dim3 grid(grid_for(nv, kBuildGrid)), block(kBlock);
    void *xd = x->d.get();
    const void *yd = y->d.get();
    if (x->dtype == SMH_F64) {
        if (sub) hipLaunchKernelGGL((k_mvec_ew<double, MvEw::Sub>), grid, block, 0, nullptr, (double *)xd, (const double *)yd, nv);
        else hipLaunchKernelGGL((k_mvec_ew<double, MvEw::Add>), grid, block, 0, nullptr, (double *)xd, (const double *)yd, nv);
    } else {
        if (sub) hipLaunchKernelGGL((k_mvec_ew<float, MvEw::Sub>), grid, block, 0, nullptr, (float *)xd, (const float *)yd, nv);
        else hipLaunchKernelGGL((k_mvec_ew<float, MvEw::Add>), grid, block, 0, nullptr, (float *)xd, (const float *)yd, nv);
    }
    SMH_HIP(hipGetLastError());
    SMH_HIP(hipStreamSynchronize(nullptr));
    return SMH_OK;
}

static int mv_pair_args(const smh_mvec *x, const smh_mvec *y) {
    if (!x || !y) return fail(SMH_ERR_INVALID, "NULL multi-vector handle");
    if (x->dtype != y->dtype) return fail(SMH_ERR_INVALID, "multi-vector dtype mismatch");
    if (x->n != y->n || x->k != y->k) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    return SMH_OK;
}

template <typename T>
static int mv_scale_t(smh_mvec *x, const double *a) {
    std::vector<T> h;
    try {
        h.assign(x->ld, T(0));
    } catch (...) {
        return fail(SMH_ERR_OOM, "host allocation failed");
    }
    for (size_t c = 0; c < x->k; ++c) h[c] = (T)a[c];
    const uint64_t nv = (uint64_t)x->n * x->ld / MvGroup<T>::N;
    if (nv == 0) return SMH_OK;
    DevArray<T> fac;
    SMH_TRY(fac.alloc(x->ld));
    SMH_HIP(hipMemcpyAsync(fac.get(), h.data(), x->ld * sizeof(T), hipMemcpyHostToDevice, nullptr));
    hipLaunchKernelGGL(k_mvec_scale<T>, dim3(grid_for(nv, kBuildGrid)), dim3(kBlock), 0, nullptr, (T *)x->d.get(), fac.get(), nv,
                       (uint32_t)(x->ld / MvGroup<T>::N), (uint32_t)x->k);
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(nullptr);  // (before the factors go back to the pool)
    SMH_HIP(e1);
    SMH_HIP(e2);
    return SMH_OK;
}

template <typename T>
static int mv_dot_t(const smh_mvec *x, const smh_mvec *y, double *out) {
    if (x->n == 0) {  // (the tree over no terms: +0)
        for (size_t c = 0; c < x->k; ++c) out[c] = 0.0;
        return SMH_OK;
    }
    const unsigned nb = mv_tree_blocks(x->n);
    DevArray<T> partials, sums;
    SMH_TRY(partials.alloc(x->ld * (size_t)nb));
    SMH_TRY(sums.alloc(x->ld));
    std::vector<T> h;
    try {
        h.resize(x->ld);
    } catch (...) {
        return fail(SMH_ERR_OOM, "host allocation failed");
    }
    auto go = [&]() -> int {
        unsigned nb2 = 0;
        SMH_TRY(mv_dot_partials_t<T>(x->d.get(), y->d.get(), x->n, x->ld, partials.get(), &nb2, nullptr));
        hipLaunchKernelGGL(k_mvec_fold<T>, dim3(mv_group_grid(x->ld)), dim3(kBlock), 0, nullptr, partials.get(), nb, (uint32_t)x->ld, sums.get());
        SMH_HIP(hipGetLastError());
        SMH_HIP(hipMemcpyAsync(h.data(), sums.get(), x->ld * sizeof(T), hipMemcpyDeviceToHost, nullptr));
        return SMH_OK;
    };
    const int rc = go();
    const hipError_t e = hipStreamSynchronize(nullptr);  // (before the workspaces go back to the pool, also after a failure)
    if (rc != SMH_OK) return keep_error(rc, [] { (void)hipGetLastError(); });
    SMH_HIP(e);
    for (size_t c = 0; c < x->k; ++c) out[c] = (double)h[c];
    return SMH_OK;
}

}  // namespace smh

using namespace smh;

extern "C" {

int smh_mvec_copy(smh_mvec *dst, const smh_mvec *src) {
    SMH_TRY(mv_pair_args(dst, src));
    const size_t bytes = src->n * src->ld * dtype_size(src->dtype);
    if (bytes == 0 || dst == src) return SMH_OK;
    SMH_HIP(hipMemcpyAsync(dst->d.get(), src->d.get(), bytes, hipMemcpyDeviceToDevice, nullptr));
    SMH_HIP(hipStreamSynchronize(nullptr));
    return SMH_OK;
}

int smh_mvec_add(smh_mvec *x, const smh_mvec *y) {
    SMH_TRY(mv_pair_args(x, y));
    return mv_addsub(x, y, false);
}

int smh_mvec_sub(smh_mvec *x, const smh_mvec *y) {
    SMH_TRY(mv_pair_args(x, y));
    return mv_addsub(x, y, true);
}

int smh_mvec_scale(smh_mvec *x, const double *a) {
    if (!x) return fail(SMH_ERR_INVALID, "NULL multi-vector handle");
    if (!a) return fail(SMH_ERR_INVALID, "NULL factor array");
    return x->dtype == SMH_F64 ? mv_scale_t<double>(x, a) : mv_scale_t<float>(x, a);
}

int smh_mvec_dot(const smh_mvec *x, const smh_mvec *y, double *out) {
    SMH_TRY(mv_pair_args(x, y));
    if (!out) return fail(SMH_ERR_INVALID, "NULL output array");
    return x->dtype == SMH_F64 ? mv_dot_t<double>(x, y, out) : mv_dot_t<float>(x, y, out);
}

int smh_mvec_norm_squared(const smh_mvec *x, double *out) { return smh_mvec_dot(x, x, out); }

}  // extern "C"
