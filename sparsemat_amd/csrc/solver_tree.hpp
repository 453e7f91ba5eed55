// solver_tree.hpp -- what the fused solvers share.  All of them (cg.hip, pcg.hip, bicgstab.hip, gmres.hip, eigsh.hip): the sweep over [0, n)
// that their element-wise kernels are written on.  Those beside cg.hip: the explicitly rounded operations, the deterministic
// workgroup sums, the one-workgroup folds of their partials and the grid of their sweeps.  The tree: a thread's own running sum, the
// __shfl_down butterfly per wave, thread 0 over the four wave sums starting from the first wave's -- tests/cg_model.py restates it
// (block_sums, from_first).  cg.hip's tree is another one (plain +, thread 0 from zero) and stays in cg.hip.
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

// thread 0 writes the workgroup's sum of a to part[blockIdx.x]
template <typename T>
__device__ __forceinline__ void block_partial(T a, T *part) {
    const T t = block_sum1(a);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// ---- folds: a strided pass over v[0..n) with p_add, then the workgroup sum ----------------------------------------------------------
template <typename T>
__device__ __forceinline__ T strided_sum(const T *__restrict__ v, uint64_t n, uint64_t first, uint64_t stride) {
    T a = T(0);
    for (uint64_t k = first; k < n; k += stride) a = p_add(a, v[k]);
    return a;
}
// one workgroup: the sum of part[0..n_parts)   (thread 0)
template <typename T>
__device__ __forceinline__ T fold1(const T *__restrict__ part, unsigned n_parts) {
    return block_sum1(strided_sum(part, n_parts, threadIdx.x, kBlock));
}
// one workgroup: the sums of part_a[0..n_parts) and part_b[0..n_parts) in out2[0], out2[1] (thread 0 writes, thread 0 reads)
template <typename T>
__device__ __forceinline__ void fold2(const T *__restrict__ part_a, const T *__restrict__ part_b, unsigned n_parts, T *out2) {
    block_sums(strided_sum(part_a, n_parts, threadIdx.x, kBlock), strided_sum(part_b, n_parts, threadIdx.x, kBlock), out2, out2 + 1);  // (blockIdx.x == 0)
}

// ---- the sweep ------------------------------------------------------------------------------------------------------------------------
// sweep<T>(n, f) runs f over [0, n) on the whole grid: thread tid = blockIdx.x * blockDim.x + threadIdx.x takes the 16-byte vectors
// q = tid, tid + threads, .. < n / V (V = 16 / sizeof(T); the arrays are 16-byte aligned), then the elements (n / V) * V + tid, ..
// < n one by one.  f is a generic lambda, written once: it is handed a position `at` with at.width (V in the body, 1 in the tail),
// at.load(ptr) and at.store(ptr, pack) for the pack of at.width values at that position of an array (ptr: the array's start; a column
// basis + c * ld with ld % V == 0 is one), and loops e = 0 .. at.width - 1 over the packs.  Accumulators are captured by reference,
// so a thread's running sum takes its elements in index order: vector lanes ascending, then the tail (cg_model.thread_sums).
// kByElement: no vectors, every element one by one.  kPlain: the vectors by ordinary loads and stores, not the non-temporal ones.
enum SweepWidth { kByElement, kBy16Bytes };
enum SweepCache { kPlain, kStreaming };

template <typename T, int W, SweepCache C>
struct SweepAt {
    static constexpr int width = W;
    typedef T pack __attribute__((ext_vector_type(W)));
    uint64_t i;  // the first element
    __device__ __forceinline__ pack load(const T *p) const {
        if constexpr (C == kStreaming) return __builtin_nontemporal_load(reinterpret_cast<const pack *>(p + i));
        else return *reinterpret_cast<const pack *>(p + i);
    }
    __device__ __forceinline__ void store(T *p, pack v) const {
        if constexpr (C == kStreaming) __builtin_nontemporal_store(v, reinterpret_cast<pack *>(p + i));
        else *reinterpret_cast<pack *>(p + i) = v;
    }
};

template <typename T, SweepWidth W = kBy16Bytes, SweepCache C = kStreaming, typename F>
__device__ __forceinline__ void sweep(uint64_t n, F &&f) {
    constexpr int V = W == kBy16Bytes ? 16 / sizeof(T) : 1;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (uint64_t)gridDim.x * blockDim.x;
    uint64_t done = 0;
    if constexpr (V > 1) {
        const uint64_t nv = n / V;
        for (uint64_t q = tid; q < nv; q += nthreads) f(SweepAt<T, V, C>{q * V});
        done = nv * V;
    }
    for (uint64_t i = done + tid; i < n; i += nthreads) f(SweepAt<T, 1, kPlain>{i});
}

// a thread's share of x.y (x may be y)
template <typename T, SweepCache C = kStreaming>
__device__ __forceinline__ T sweep_dot(const T *x, const T *y, uint64_t n) {
    T a = T(0);
    sweep<T, kBy16Bytes, C>(n, [&](auto at) {
        const auto xv = at.load(x), yv = at.load(y);
#pragma unroll
        for (int e = 0; e < at.width; ++e) a = p_add(a, p_mul(xv[e], yv[e]));
    });
    return a;
}

inline unsigned pcg_grid(size_t n) {
    uint64_t b = (n + kBlock - 1) / kBlock;
    if (b > (uint64_t)kPcgBlocks) b = kPcgBlocks;
    return (unsigned)(b ? b : 1);
}

}  // namespace smh
