// Stand-in for csrc/internal.hpp that lets tests/cpp/k1m_on_host.cpp compile the SOURCE of spmv_many.hip for the host: a workgroup is
// 256 std::threads and a std::barrier, workgroups run one after the other, hipLaunchKernelGGL runs the grid right away.  Host
// compilers see every index the kernel computes, so AddressSanitizer and UBSan check its bounds on exact-size arrays -- on a
// CPU, where a stray access costs nothing.  (clang only: the kernels use ext_vector_type.)
#pragma once
#include <algorithm>
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>
#define SMH_OK 0
#define SMH_F32 0
#define SMH_F64 1
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)
#define __restrict__
struct Idx { unsigned x; };
struct dim3 { unsigned x; dim3(unsigned v = 1) : x(v) {} };
inline thread_local Idx threadIdx;
inline Idx blockIdx, gridDim;
inline std::barrier<> *g_bar = nullptr;
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline float __fmul_rn(float a, float b) { return a * b; }
inline float __fadd_rn(float a, float b) { return a + b; }
inline double __dmul_rn(double a, double b) { return a * b; }
inline double __dadd_rn(double a, double b) { return a + b; }
using std::min; using std::max;
typedef void *hipStream_t;
#define SMH_HIP(x) (void)0
inline int hipGetLastError() { return 0; }
template <typename F> void cpu_launch(unsigned grid, unsigned block, F f) {
    gridDim.x = grid;
    for (unsigned b = 0; b < grid; ++b) {
        blockIdx.x = b;
        std::barrier<> bar(block);
        g_bar = &bar;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < block; ++t) th.emplace_back([&, t] { threadIdx.x = t; f(); });
        for (auto &x : th) x.join();
    }
}
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) cpu_launch((grid).x, (block).x, [&] { kern(__VA_ARGS__); })
namespace smh {
constexpr int kWave = 64, kBlock = 256, kStreamRows = 256, kManyCap = 2048;
}
