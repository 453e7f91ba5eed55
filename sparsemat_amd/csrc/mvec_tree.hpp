// mvec_tree.hpp -- what the multi-vector BLAS-1 (mvec_blas.hip) and the k-column solver (cg_many.hip) share: the 16-byte row
// group, the rounded element-wise operations, and the workgroup stage of the column tree.
#pragma once
#include "internal.hpp"

namespace smh {

// a row group: the columns of one row that one 16-byte load holds
template <typename T> struct MvGroup;
template <> struct MvGroup<float> { typedef float type __attribute__((ext_vector_type(4))); static constexpr int N = 4; };
template <> struct MvGroup<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int N = 2; };

__device__ __forceinline__ float mv_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mv_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float mv_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double mv_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ float mv_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double mv_sub(double a, double b) { return __dsub_rn(a, b); }

// The workgroup sums of G per-thread values at once, each as cg.hip's cg_block_sum builds one: a wavefront folds by __shfl_down
// (32, 16, ..., 1), then ONE thread adds the four wave sums in order from T(0).  s_sum[e] holds them, for every thread, on return.
template <typename T, int G>
__device__ __forceinline__ void mv_block_sums(T (&v)[G], T (*s_w)[kBlock / kWave], T *s_sum) {
#pragma unroll
    for (int e = 0; e < G; ++e) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) v[e] += __shfl_down(v[e], o, kWave);
    }
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < G; ++e) s_w[e][wave] = v[e];
    }
    __syncthreads();
    if (threadIdx.x < G) {
        T r = T(0);
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) r += s_w[threadIdx.x][w];
        s_sum[threadIdx.x] = r;
    }
    __syncthreads();
}

// s_sum[e] = the fold of the nb partials of column col0 + e (partials[c * nb + i]): thread t adds partial[t], partial[t + 256], ...
// from T(0), then the workgroup sum -- every workgroup that runs it gets the same bits
template <typename T, int G>
__device__ __forceinline__ void mv_fold_group(const T *__restrict__ partials, uint32_t nb, uint32_t col0, T (*s_w)[kBlock / kWave], T *s_sum) {
    T acc[G];
#pragma unroll
    for (int e = 0; e < G; ++e) {
        acc[e] = T(0);
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) acc[e] += partials[(uint64_t)(col0 + e) * nb + i];
    }
    mv_block_sums<T, G>(acc, s_w, s_sum);
}

// workgroups per row group of a column-tree sweep over n rows: min(reduce_blocks(n), 512)   (mvec_blas.hip)
unsigned mv_tree_blocks(size_t n);
// partials[c * *nb_out + w] of x_c . y_c for every column c < ld, enqueued on s; partials: ld * mv_tree_blocks(n) values
int mv_dot_partials(int dtype, const void *x, const void *y, size_t n, size_t ld, void *partials, unsigned *nb_out, hipStream_t s);
// r = b - r over the whole storage (one rounding), enqueued on s
int mv_rsub_into(int dtype, void *r, const void *b, size_t n, size_t ld, hipStream_t s);

}  // namespace smh
