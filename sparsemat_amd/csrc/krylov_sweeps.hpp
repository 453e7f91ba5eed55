// krylov_sweeps.hpp -- the classical Gram-Schmidt sweeps over a device-resident basis, written once for gmres.hip and eigsh.hip:
// all v_c.w of a pass in one launch (dots), their folds, and the update of w by the columns ascending.  The basis is columns of
// stride ld (ld % V == 0), every column a vector that solver_tree.hpp's sweep reads by 16 bytes.  A solver keeps its state on the
// device and hands these kernels three pointers into it: `due` (a word: 0 = this launch returns at once -- bodies enqueued past a
// stop are no-ops), `j` (columns v_0 .. v_j take part) and the coefficient array h of the pass.
// The dots: w's pack is loaded once per tile of kGsTile = 8 columns, one accumulator per column; every column is summed by
// solver_tree.hpp's tree on pcg_grid(n) -- cg_model.Reducer.dot(., ., "pcg") -- so the tile width changes no bit.
#pragma once
#include "internal.hpp"
#include "solver_tree.hpp"

namespace smh {

constexpr int kGsTile = 8;  // columns per load of w in the dots (no bit depends on it)

template <typename T> __device__ __forceinline__ T p_sqrt(T a) { return (T)sqrt((double)a); }  // (f64's sqrt rounds an f32 correctly too)

// partials of v_c.w for c = 0 .. j: part[c * kPcgBlocks + block]
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_gs_dots(const uint32_t *__restrict__ due, const uint32_t *__restrict__ j, const T *__restrict__ basis, uint64_t ld, const T *__restrict__ w,
          uint64_t n, T *__restrict__ part) {
    if (!*due) return;  // block-uniform
    const unsigned ncols = *j + 1;
    __shared__ T sa[kGsTile][kBlock / kWave];
    for (unsigned c0 = 0; c0 < ncols; c0 += kGsTile) {
        const unsigned width = ncols - c0 < (unsigned)kGsTile ? ncols - c0 : (unsigned)kGsTile;
        const T *col0 = basis + (uint64_t)c0 * ld;
        T acc[kGsTile];
#pragma unroll
        for (int t = 0; t < kGsTile; ++t) acc[t] = T(0);
        sweep<T>(n, [&](auto at) {
            const auto wv = at.load(w);
#pragma unroll
            for (int t = 0; t < kGsTile; ++t) {
                if ((unsigned)t < width) {
                    const auto vv = at.load(col0 + (uint64_t)t * ld);
#pragma unroll
                    for (int e = 0; e < at.width; ++e) acc[t] = p_add(acc[t], p_mul(vv[e], wv[e]));
                }
            }
        });
        // solver_tree.hpp's workgroup sum written out for a tile: one accumulator per column, and thread t < width (not thread 0)
        // sums and writes column t -- block_sum1 per column would cost a barrier each, so this stays its own
#pragma unroll
        for (int t = 0; t < kGsTile; ++t) {
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1) acc[t] = p_add(acc[t], (T)__shfl_down(acc[t], o, kWave));
            if ((threadIdx.x & (kWave - 1)) == 0) sa[t][threadIdx.x / kWave] = acc[t];
        }
        __syncthreads();
        if (threadIdx.x < width) {
            T s = sa[threadIdx.x][0];
            for (int wv = 1; wv < kBlock / kWave; ++wv) s = p_add(s, sa[threadIdx.x][wv]);
            part[(uint64_t)(c0 + threadIdx.x) * kPcgBlocks + blockIdx.x] = s;
        }
        __syncthreads();  // (sa is written again by the next tile)
    }
}

// workgroup c folds column c's partials into h_c; launched on as many workgroups as the basis has columns
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_gs_fold(const uint32_t *__restrict__ due, const uint32_t *__restrict__ j, T *__restrict__ h, const T *__restrict__ part, unsigned n_parts) {
    if (!*due || blockIdx.x > *j) return;
    const T hc = fold1(part + (uint64_t)blockIdx.x * kPcgBlocks, n_parts);
    if (threadIdx.x == 0) h[blockIdx.x] = hc;
}

// w = (..((w - v_0 h_0) - v_1 h_1) .. - v_j h_j); WW: and the partials of w.w
template <typename T, bool WW>
__global__ void __launch_bounds__(kBlock)
k_gs_update(const uint32_t *__restrict__ due, const uint32_t *__restrict__ j, const T *__restrict__ h, const T *__restrict__ basis, uint64_t ld,
            T *__restrict__ w, uint64_t n, T *__restrict__ part_ww) {
    if (!*due) return;
    const unsigned ncols = *j + 1;
    T acc = T(0);
    sweep<T>(n, [&](auto at) {
        auto wv = at.load(w);
#pragma unroll 8
        for (unsigned c = 0; c < ncols; ++c) {
            const auto vv = at.load(basis + (uint64_t)c * ld);
            const T hc = h[c];
#pragma unroll
            for (int e = 0; e < at.width; ++e) wv[e] = p_add(wv[e], -p_mul(vv[e], hc));
        }
        if (WW) {
#pragma unroll
            for (int e = 0; e < at.width; ++e) acc = p_add(acc, p_mul(wv[e], wv[e]));
        }
        at.store(w, wv);
    });
    if (WW) block_partial(acc, part_ww);
}

}  // namespace smh
