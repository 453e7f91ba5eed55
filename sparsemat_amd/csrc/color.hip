// color.hip -- a multicolour ordering of a square CRS pattern on the device (DESIGN.md "Multicolour ordering"), so that a general
// matrix gets few levels in its triangular solves without its caller knowing a colouring.  EXTENSION: the reference has no ordering;
// the known answer is the numpy model tests/color_model.py, which the result equals exactly.
//
// Definition.  The graph is reorder.hip's: vertices 0..n-1; u ~ v iff u != v and an entry (u, v) or (v, u) is stored (stored zeros
// count, duplicates once; values are never read); deg(v) = number of distinct neighbours.  h(v) = mix(v XOR seed) on 32 bits, mix the
// bijection x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.  The priority of v is the 64-bit key
// deg(v) << 32 | h(v): all keys are distinct.  Visiting the vertices in DESCENDING key order, each takes the smallest colour >= 0 that
// no neighbour of higher key holds (sequential greedy: n_colors <= max deg + 1).  round(v) = 0 when no neighbour has a higher key, else
// 1 + max round(w) over the neighbours w of higher key; n_rounds = 1 + max round.  perm[new] = old is the vertices sorted by
// (colour, index).
//
// Set-up (once): the symmetrised pattern adj_off / adj_col (symmetrised_pattern, shared with the RCM ordering), then the keys in an
// array of their own: 8 bytes per vertex, which spare every neighbour test two offset loads.
//
// A round (the Jones-Plassmann schedule of that colouring; the round boundary is the kernel boundary; no kernel waits on another
// workgroup, nothing is polled, there are no flags and no spins, the only atomics are integer add / max):
//   k_color_round    round k colours every vertex of the worklist that has no colour yet and whose higher-key neighbours were all
//                    coloured in an EARLIER round: stamp[w] holds the round that coloured w, and a stamp read as "none" or as k itself
//                    fails the test alike, so the vertices of one round cannot see each other -- only with that is n_rounds the
//                    definition's number whatever the scheduling.  A vertex that passes collects its higher neighbours' colours into a
//                    64-bit mask of the window [base, base + kColorWindow) and takes the first free bit; a full window moves the base
//                    and walks the list again.  A thread walks a list of up to kColorThreadDeg neighbours itself (its smallest free
//                    colour is at most its degree: one window always suffices); a longer list is walked by the whole workgroup.
//   The rounds run over a worklist of the vertices without a colour.  k_color_compact rewrites it at the end of a batch of rounds
//   (the order inside it is free: no result depends on it), and the host reads ONE small block per batch -- the vertices each round
//   coloured, the new worklist length, the largest colour -- with batches of kColorFirstBatch, then twice as many rounds up to
//   kColorMaxBatch.  A round enqueued after the last vertex was coloured finds every stamp set and does nothing.  Every round before
//   that colours the uncoloured vertex of the largest key at least, so a batch that colours nothing is an error, not a loop.
// The permutation is ONE stable radix sort of 0 .. n-1 by colour, bits_for(n_colors - 1) bits wide.
//
// Memory: the set-up's (reorder.hip), then 8 bytes per distinct neighbour pair plus 28 per vertex (keys 8, stamp 4, colour 4, two
// worklists 8, the offsets 4).
#include <rocprim/device/device_radix_sort.hpp>

#include <chrono>
#include <cstdlib>

#include "arg_stage.hpp"

namespace smh {

namespace {

constexpr uint32_t kNoStamp = 0xFFFFFFFFu;
constexpr int kColorBlock = kBlock;          // lane width: worklist vertices a workgroup takes per sweep, and the lanes that walk a long list together
constexpr uint32_t kColorThreadDeg = 32;     // longest neighbour list one thread of k_color_round walks by itself
constexpr uint32_t kColorWindow = 64;        // colours one mask holds
constexpr uint64_t kColorGrid = 4096;        // workgroups of a round at most (twice what the chip holds at once): a longer worklist takes several sweeps of kColorGrid * kColorBlock vertices
constexpr size_t kColorFirstBatch = 4;       // rounds before the first read-back; every batch after it has twice as many ...
constexpr size_t kColorMaxBatch = 64;        // ... up to this
constexpr int kCtlNext = (int)kColorMaxBatch;  // ctl: [0, kColorMaxBatch) vertices coloured by each round of the batch, then the next worklist's length ...
constexpr int kCtlMax = kCtlNext + 1;          // ... and the largest colour so far (kept across batches)
constexpr int kCtlWords = kCtlMax + 1;
static_assert(kColorWindow == 64, "the mask is one 64-bit word");
static_assert(kColorThreadDeg < kColorWindow, "a thread-walked vertex must find its colour in the first window");

__device__ __forceinline__ uint32_t color_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__global__ void __launch_bounds__(kBlock)
k_color_init(const uint32_t *__restrict__ adj_off, uint64_t n, uint32_t seed, uint64_t *__restrict__ keys, uint32_t *__restrict__ worklist) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
        keys[v] = ((uint64_t)(adj_off[v + 1] - adj_off[v]) << 32) | color_mix((uint32_t)v ^ seed);
        worklist[v] = (uint32_t)v;
    }
}

__global__ void __launch_bounds__(kBlock) k_color_iota(uint32_t *out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = (uint32_t)i;
}

// the OR of a mask over the wavefront, in every lane
__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long m) {
    uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo |= (uint32_t)__shfl_xor((int)lo, o, kWave);
        hi |= (uint32_t)__shfl_xor((int)hi, o, kWave);
    }
    return ((unsigned long long)hi << 32) | lo;
}

// one round over the worklist; *cnt += vertices it coloured, *max_color = max(the colours it gave)
__global__ void __launch_bounds__(kColorBlock)
k_color_round(const uint32_t *__restrict__ worklist, uint64_t n_work, const uint32_t *__restrict__ adj_off, const uint32_t *__restrict__ adj_col,
              const uint64_t *__restrict__ keys, uint32_t round, uint32_t *stamp, uint32_t *color, uint32_t *cnt, uint32_t *max_color) {
    __shared__ uint32_t s_long[kColorBlock];
    __shared__ uint32_t s_nlong;
    __shared__ unsigned long long s_mask[kColorBlock / kWave];
    if (threadIdx.x == 0) s_nlong = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t my_cnt = 0, my_max = 0;  // the vertices this thread coloured, and the largest colour it gave
    for (uint64_t base = (uint64_t)blockIdx.x * kColorBlock; base < n_work; base += (uint64_t)gridDim.x * kColorBlock) {  // (uniform trip count)
        const uint64_t i = base + threadIdx.x;
        bool took = false;
        uint32_t mine = 0;
        if (i < n_work) {
            const uint32_t v = worklist[i];
            if (stamp[v] == kNoStamp) {
                const uint32_t b = adj_off[v], e = adj_off[v + 1];
                if (e - b <= kColorThreadDeg) {
                    const uint64_t kv = keys[v];
                    // the test first, over the whole list without an early exit and with both gathers unconditional: the iterations
                    // are independent, so their loads overlap (measured: the same time as a loop that left at the first waiting
                    // neighbour); the colours are gathered only by the vertices that pass
                    bool wait = false;
#pragma unroll 4
                    for (uint32_t q = b; q < e; ++q) {
                        const uint32_t w = adj_col[q];
                        const bool higher = keys[w] > kv, open = stamp[w] >= round;  // no colour yet, or one of this very round
                        wait |= higher & open;
                    }
                    took = !wait;
                    if (took) {
                        unsigned long long mask = 0;
#pragma unroll 4
                        for (uint32_t q = b; q < e; ++q) {
                            const uint32_t w = adj_col[q];
                            const uint32_t c = color[w];  // (a neighbour of lower key: no colour yet, or one that is not looked at)
                            if (keys[w] > kv && c < kColorWindow) mask |= 1ull << c;
                        }
                        mine = (uint32_t)__ffsll((long long)~mask) - 1;  // (at most e - b <= kColorThreadDeg bits are set)
                        color[v] = mine;
                        stamp[v] = round;
                    }
                } else {
                    s_long[atomicAdd(&s_nlong, 1u)] = v;
                }
            }
        }
        if (took) {
            ++my_cnt;
            my_max = mine > my_max ? mine : my_max;
        }
        __syncthreads();
        const uint32_t nl = s_nlong;
        for (uint32_t j = 0; j < nl; ++j) {  // the long lists, one after the other, by all threads
            const uint32_t v = s_long[j];
            const uint32_t b = adj_off[v], e = adj_off[v + 1];
            const uint64_t kv = keys[v];
            int wait = 0;
            for (uint64_t q = (uint64_t)b + threadIdx.x; q < e; q += kColorBlock) {
                const uint32_t w = adj_col[q];
                if (keys[w] > kv && stamp[w] >= round) wait = 1;
            }
            if (__syncthreads_or(wait)) continue;  // (uniform)
            uint32_t found = kNoStamp;
            for (uint32_t lo = 0; lo <= e - b; lo += kColorWindow) {  // the smallest free colour is at most the degree
                unsigned long long mask = 0;
                for (uint64_t q = (uint64_t)b + threadIdx.x; q < e; q += kColorBlock) {
                    const uint32_t w = adj_col[q];
                    if (keys[w] > kv) {
                        const uint32_t c = color[w] - lo;  // (a colour below the window wraps to a large number)
                        if (c < kColorWindow) mask |= 1ull << c;
                    }
                }
                mask = wave_or_u64(mask);
                if (lane == 0) s_mask[wave] = mask;
                __syncthreads();
                unsigned long long all = 0;
#pragma unroll
                for (int k = 0; k < kColorBlock / kWave; ++k) all |= s_mask[k];
                __syncthreads();  // (nobody writes s_mask again before everybody has read it)
                if (all != ~0ull) {
                    found = lo + (uint32_t)__ffsll((long long)~all) - 1;
                    break;  // (uniform: every thread holds the same mask)
                }
            }
            if (threadIdx.x == 0 && found != kNoStamp) {
                color[v] = found;
                stamp[v] = round;
                ++my_cnt;
                my_max = found > my_max ? found : my_max;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) s_nlong = 0;
        __syncthreads();
    }
    // what this wavefront coloured over all its sweeps, in ONE add and ONE max (per wavefront and sweep they were half a million
    // atomics on one address in a round over 16.8 M vertices, and those, not the gathers, were the round's time)
    const uint32_t top = wave_max_u32(my_cnt ? my_max : 0u);
    uint32_t sum = my_cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += (uint32_t)__shfl_xor((int)sum, o, kWave);
    if (lane == 0 && sum) {
        atomicAdd(cnt, sum);
        atomicMax(max_color, top);
    }
}

// the vertices of the worklist that still have no colour, in any order; *n_out += their number
__global__ void __launch_bounds__(kBlock)
k_color_compact(const uint32_t *__restrict__ worklist, uint64_t n_work, const uint32_t *__restrict__ stamp, uint32_t *__restrict__ out, uint32_t *n_out) {
    const unsigned lane = threadIdx.x & (kWave - 1);
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n_work; base += (uint64_t)gridDim.x * kBlock) {  // (uniform trip count)
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < n_work ? worklist[i] : 0u;
        const bool keep = i < n_work && stamp[v] == kNoStamp;
        const unsigned long long kept = __ballot(keep);
        if (!kept) continue;  // (uniform over the wavefront)
        const int leader = __ffsll((long long)kept) - 1;
        uint32_t at = 0;
        if ((int)lane == leader) at = atomicAdd(n_out, (uint32_t)__popcll(kept));
        at = (uint32_t)__shfl((int)at, leader, kWave);
        if (keep) out[at + (uint32_t)__popcll(kept & ((1ull << lane) - 1ull))] = v;
    }
}

}  // namespace

// colors_out / perm_out: device arrays of n entries, either may be null.  off / col: a square pattern of n rows whose columns are all
// below n (the caller's checks).
int color_order(const uint32_t *off, const uint32_t *col, size_t n, size_t nnz, uint32_t seed, uint32_t *colors_out, uint32_t *perm_out, size_t *n_colors,
                size_t *n_rounds, hipStream_t s) {
    *n_colors = *n_rounds = 0;
    if (n == 0) return SMH_OK;
    // SMH_COLOR_TRACE=1 (development aid): the stages' wall times, each behind a stream synchronisation, on stderr
    static const bool trace = getenv("SMH_COLOR_TRACE") && atoi(getenv("SMH_COLOR_TRACE")) != 0;
    auto t_last = std::chrono::steady_clock::now();
    auto stage = [&](const char *what, size_t a, size_t b) {
        if (!trace) return;
        (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[color] %-28s %8.3f ms  (%zu, %zu)\n", what, std::chrono::duration<double, std::milli>(now - t_last).count(), a, b);
        t_last = now;
    };
    Scratch scr;
    uint32_t *adj_off = nullptr, *adj_col = nullptr;
    SMH_TRY(symmetrised_pattern(off, col, n, nnz, scr, &adj_off, &adj_col, s));
    stage("symmetrised pattern", n, nnz);
    uint64_t *keys = nullptr;
    uint32_t *stamp = nullptr, *color = colors_out, *work = nullptr, *work_next = nullptr, *ctl = nullptr;
    SMH_TRY(scr.alloc(&keys, n));
    SMH_TRY(scr.alloc(&stamp, n));
    if (!color) SMH_TRY(scr.alloc(&color, n));
    SMH_TRY(scr.alloc(&work, n));
    SMH_TRY(scr.alloc(&work_next, n));
    SMH_TRY(scr.alloc(&ctl, kCtlWords));
    const unsigned grid_n = grid_for(n, kBuildGrid);
    SMH_HIP(hipMemsetAsync(stamp, 0xFF, n * sizeof(uint32_t), s));
    SMH_HIP(hipMemsetAsync(color, 0xFF, n * sizeof(uint32_t), s));
    SMH_HIP(hipMemsetAsync(ctl, 0, kCtlWords * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_color_init, dim3(grid_n), dim3(kBlock), 0, s, adj_off, (uint64_t)n, seed, keys, work);
    SMH_HIP(hipGetLastError());
    stage("keys, worklist", n, 0);
    uint32_t h_ctl[kCtlWords];
    size_t done = 0, round = 0, batch = kColorFirstBatch, n_work = n;
    while (done < n) {
        const size_t left = n - done, rounds = batch < left ? batch : left;  // (every round colours a vertex: `left` rounds always suffice)
        const unsigned grid = grid_for(n_work, kColorGrid);
        for (size_t k = 0; k < rounds; ++k)
            hipLaunchKernelGGL(k_color_round, dim3(grid), dim3(kColorBlock), 0, s, work, (uint64_t)n_work, adj_off, adj_col, keys, (uint32_t)(round + k), stamp, color,
                               ctl + k, ctl + kCtlMax);
        SMH_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_color_compact, dim3(grid_for(n_work, kBuildGrid)), dim3(kBlock), 0, s, work, (uint64_t)n_work, stamp, work_next, ctl + kCtlNext);
        SMH_HIP(hipGetLastError());
        SMH_HIP(hipMemcpyAsync(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, s));
        SMH_HIP(hipMemsetAsync(ctl, 0, kCtlMax * sizeof(uint32_t), s));  // (the counts and the length; the largest colour stays)
        SMH_HIP(hipStreamSynchronize(s));
        size_t colored = 0;
        for (size_t k = 0; k < rounds; ++k) {
            if (h_ctl[k] == 0) continue;
            if (done + colored >= n || (k > 0 && h_ctl[k - 1] == 0))
                return fail(SMH_ERR_INVALID, "colouring: round %zu coloured %u vertices after a round that coloured none", round + k, h_ctl[k]);
            colored += h_ctl[k];
            *n_rounds = round + k + 1;
        }
        if (colored == 0) return fail(SMH_ERR_INVALID, "colouring: no progress in rounds %zu .. %zu with %zu of %zu vertices coloured", round, round + rounds - 1, done, n);
        done += colored;
        if (done > n || h_ctl[kCtlNext] != n - done)
            return fail(SMH_ERR_INVALID, "colouring: %zu of %zu vertices coloured but %u left on the worklist", done, n, h_ctl[kCtlNext]);
        stage("a batch: rounds, worklist", rounds, n_work);
        n_work = n - done;
        std::swap(work, work_next);
        round += rounds;
        if (batch < kColorMaxBatch) batch *= 2;
    }
    *n_colors = (size_t)h_ctl[kCtlMax] + 1;
    if (perm_out) {  // the vertices by (colour, index): a stable sort of 0 .. n-1 by colour
        hipLaunchKernelGGL(k_color_iota, dim3(grid_n), dim3(kBlock), 0, s, work, (uint64_t)n);
        SMH_HIP(hipGetLastError());
        SMH_ROCPRIM(s, rocprim::radix_sort_pairs(tmp, bytes, color, work_next, work, perm_out, n, 0u, bits_for(*n_colors - 1), s));
    }
    SMH_HIP(hipStreamSynchronize(s));
    stage("sort by colour", *n_colors, *n_rounds);
    return SMH_OK;
}

// ---- the entry points ----------------------------------------------------------------------------------------------------------
static int color_common(const smh_crs *m, uint32_t seed, uint32_t *colors_out, uint32_t *perm_out, size_t *n_colors_out, size_t *n_rounds_out,
                        bool on_device) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (m->n_rows != m->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    SMH_TRY(columns_within_n_cols(m, "color"));
    const size_t n = m->n_rows;
    ArgStage st(on_device, m->device);
    void *d_colors = nullptr, *d_perm = nullptr;  // (either may be NULL: that output is not wanted)
    SMH_TRY(st.out(colors_out, n * sizeof(uint32_t), "colors_out", &d_colors));
    SMH_TRY(st.out(perm_out, n * sizeof(uint32_t), "perm_out", &d_perm));
    SMH_TRY(st.callers_writes_first());
    SMH_HIP(hipStreamSynchronize(m->stream));
    size_t colors = 0, rounds = 0;
    SMH_TRY(color_order(m->d_off, m->d_col, n, m->nnz, seed, (uint32_t *)d_colors, (uint32_t *)d_perm, &colors, &rounds, m->stream));
    SMH_TRY(st.finish());
    if (n_colors_out) *n_colors_out = colors;
    if (n_rounds_out) *n_rounds_out = rounds;
    return SMH_OK;
}

}  // namespace smh

using namespace smh;

extern "C" {

int smh_crs_color(const smh_crs *m, uint32_t seed, uint32_t *colors_out, uint32_t *perm_out, size_t *n_colors_out, size_t *n_rounds_out) {
    return color_common(m, seed, colors_out, perm_out, n_colors_out, n_rounds_out, false);
}
int smh_crs_color_dev(const smh_crs *m, uint32_t seed, uint32_t *colors_out_dev, uint32_t *perm_out_dev, size_t *n_colors_out, size_t *n_rounds_out) {
    return color_common(m, seed, colors_out_dev, perm_out_dev, n_colors_out, n_rounds_out, true);
}

}  // extern "C"
