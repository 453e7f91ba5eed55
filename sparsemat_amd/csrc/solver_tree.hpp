// solver_tree.hpp -- what the fused solvers beside cg.hip share (pcg.hip, bicgstab.hip): the explicitly rounded operations, the
// deterministic workgroup sums and the grid of their sweeps.  The tree: a thread's own running sum, the __shfl_down butterfly per
// wave, thread 0 over the four wave sums starting from the first wave's -- tests/cg_model.py restates it (block_sums, from_first).
#pragma once
#include "internal.hpp"

namespace smh {

constexpr int kPcgBlocks = 512;  // 2 blocks per CU (the CG tail's measured optimum)

template <typename T> __device__ __forceinline__ T p_mul(T a, T b) { if constexpr (sizeof(T) == 4) return __fmul_rn(a, b); else return __dmul_rn(a, b); }
template <typename T> __device__ __forceinline__ T p_add(T a, T b) { if constexpr (sizeof(T) == 4) return __fadd_rn(a, b); else return __dadd_rn(a, b); }
template <typename T> __device__ __forceinline__ T p_div(T a, T b) { if constexpr (sizeof(T) == 4) return __fdiv_rn(a, b); else return __ddiv_rn(a, b); }

// workgroup sums of a and b: thread 0 writes them to pa[blockIdx.x], pb[blockIdx.x]
template <typename T>
__device__ __forceinline__ void block_sums(T a, T b, T *pa, T *pb) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        a = p_add(a, (T)__shfl_down(a, o, kWave));
        b = p_add(b, (T)__shfl_down(b, o, kWave));
    }
    __shared__ T sa[kBlock / kWave], sb[kBlock / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) { sa[threadIdx.x / kWave] = a; sb[threadIdx.x / kWave] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        T ta = sa[0], tb = sb[0];
        for (int w = 1; w < kBlock / kWave; ++w) { ta = p_add(ta, sa[w]); tb = p_add(tb, sb[w]); }
        pa[blockIdx.x] = ta;
        pb[blockIdx.x] = tb;
    }
}

template <typename T>
__device__ __forceinline__ T block_sum1(T a) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) a = p_add(a, (T)__shfl_down(a, o, kWave));
    __shared__ T sa1[kBlock / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) sa1[threadIdx.x / kWave] = a;
    __syncthreads();
    T t = T(0);
    if (threadIdx.x == 0) {
        t = sa1[0];
        for (int w = 1; w < kBlock / kWave; ++w) t = p_add(t, sa1[w]);
    }
    return t;  // (thread 0)
}

inline unsigned pcg_grid(size_t n) {
    uint64_t b = (n + kBlock - 1) / kBlock;
    if (b > (uint64_t)kPcgBlocks) b = kPcgBlocks;
    return (unsigned)(b ? b : 1);
}

}  // namespace smh
