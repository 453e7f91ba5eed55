// reorder.hip -- the reverse Cuthill-McKee ordering of a square CRS pattern on the device (DESIGN.md "Reordering").
// EXTENSION: the reference has no ordering; the known answer is the numpy model tests/reorder_model.py, which the result
// equals exactly.
//
// Definition.  Vertices 0..n-1; u ~ v iff u != v and an entry (u, v) or (v, u) is stored (stored zeros count, duplicates
// once; values are never read); deg(v) = number of distinct neighbours.  While unvisited vertices remain, the root is the
// unvisited vertex with the smallest (deg, index) -- so all isolated vertices come first, in index order, and are emitted in
// one step.  From the root level by level: the next level is the set of unvisited neighbours of the current one, each new
// vertex v keyed by (position in the order of its earliest-placed parent, deg(v), v), appended in ascending key order.  The
// result is that order reversed.  n_components counts roots, n_levels counts levels over all components, root levels included.
//
// Set-up (once; symmetrised_pattern, which the multicolour ordering of color.hip shares): both directions of every off-diagonal entry as 64-bit keys (row << 32 | column; diagonal entries become a key
// in row n, past every vertex), one radix sort, the distinct keys compacted by the library's scan -> the symmetrised pattern
// adj_off / adj_col with ascending neighbour lists; the vertices sorted by (deg, index) for the root search.
//
// A level (the level boundary is the kernel boundary; no kernel waits on another workgroup, nothing is polled, the only
// atomics are integer min / add):
//   k_rcm_expand     every frontier vertex (position p in the order) offers p to its neighbours with atomicMin on parent[]: the
//                    outcome is the smallest offering position whatever the arrival order.  The one offer that finds parent[]
//                    unset appends the vertex to the candidate list (its slot there is arbitrary; the sort below removes that).
//                    Placed vertices hold a position below every later offer, so no visited flags are needed.  A thread walks
//                    a frontier vertex of up to kRcmThreadDeg neighbours itself; longer lists are walked by the whole workgroup.
//   [host reads the candidate count: the one small block per level]
//   two stable radix sorts (rocPRIM): the candidates by index, then by (parent position - level start, deg) -- together the
//   full key, every key distinct, so the level's order is fixed.
//   k_rcm_place      appends the level to the order.
// A component starts with k_rcm_find_root: ONE workgroup walks the (deg, index)-sorted vertices from where the last root was
// found to the first unvisited one -- the walk never goes back, n steps over the whole run.
//
// Cost: one round (a handful of launches and one 16-byte read-back) per level, plus one per component; each round places at
// least one vertex or ends its component, so the host loop runs at most n_levels + n_components rounds.  A chain of n vertices
// takes n rounds.  Memory: 40 bytes per stored entry during the set-up, 8 per distinct neighbour pair plus 24 per vertex after it.
#include <rocprim/device/device_radix_sort.hpp>

#include "arg_stage.hpp"
#include "crs_forms.hpp"

namespace smh {

namespace {

constexpr uint32_t kUnset = 0xFFFFFFFFu;
constexpr uint32_t kRcmThreadDeg = 32;   // longest neighbour list one thread of k_rcm_expand walks by itself
constexpr int kRcmRootBlock = 1024;      // threads of the root search
constexpr uint64_t kRcmExpandGrid = 1024;  // workgroups of k_rcm_expand at most: a wider level takes several sweeps of kRcmExpandGrid * kBlock vertices

__global__ void __launch_bounds__(kBlock)
k_rcm_keys(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ col, uint64_t nnz, uint64_t n, uint64_t *__restrict__ keys) {
    const uint64_t none = n << 32;  // sorts behind every vertex's keys
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t u = rows[e], v = col[e];
        keys[2 * e] = u != v ? (u << 32) | v : none;
        keys[2 * e + 1] = u != v ? (v << 32) | u : none;
    }
}

__device__ __forceinline__ bool rcm_is_head(const uint64_t *keys, uint64_t k, uint64_t n) {
    const uint64_t key = keys[k];
    return (key >> 32) < n && (k == 0 || keys[k - 1] != key);
}

__global__ void __launch_bounds__(kBlock)
k_rcm_heads(const uint64_t *__restrict__ keys, uint64_t m2, uint64_t n, uint32_t *__restrict__ pos) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= m2; k += (uint64_t)gridDim.x * blockDim.x)
        pos[k] = k < m2 && rcm_is_head(keys, k, n) ? 1u : 0u;
}

__global__ void __launch_bounds__(kBlock)
k_rcm_adj_col(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ pos, uint64_t m2, uint64_t n, uint32_t *__restrict__ adj_col) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m2; k += (uint64_t)gridDim.x * blockDim.x)
        if (rcm_is_head(keys, k, n)) adj_col[pos[k]] = (uint32_t)keys[k];
}

// adj_off[v] = distinct keys in front of vertex v's first one; deg, the identity for the (deg, index) sort, the isolated count
__global__ void __launch_bounds__(kBlock)
k_rcm_adj_off(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ pos, uint64_t m2, uint64_t n, uint32_t *__restrict__ adj_off) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= n; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t want = v << 32;
        uint64_t lo = 0, hi = m2;  // first k with keys[k] >= want
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < want) lo = mid + 1; else hi = mid;
        }
        adj_off[v] = pos[lo];  // (pos[m2] = number of distinct keys)
    }
}

__global__ void __launch_bounds__(kBlock)
k_rcm_degrees(const uint32_t *__restrict__ adj_off, uint64_t n, uint32_t *__restrict__ deg, uint32_t *__restrict__ iota, uint32_t *__restrict__ stats2) {
    uint32_t iso = 0, mx = 0;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t d = adj_off[v + 1] - adj_off[v];
        deg[v] = d;
        iota[v] = (uint32_t)v;
        iso += d == 0;
        mx = d > mx ? d : mx;
    }
    if (iso) atomicAdd(&stats2[0], iso);
    if (mx) atomicMax(&stats2[1], mx);
}

__global__ void __launch_bounds__(kBlock)
k_rcm_place_isolated(const uint32_t *__restrict__ by_deg, uint64_t n_iso, uint32_t *__restrict__ order, uint32_t *__restrict__ parent) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_iso; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t v = by_deg[i];
        order[i] = v;
        parent[v] = (uint32_t)i;
    }
}

// ctl: [0] candidates appended by the expansion, [1] where in by_deg the root was found
__global__ void __launch_bounds__(kRcmRootBlock)
k_rcm_find_root(const uint32_t *__restrict__ by_deg, uint32_t *__restrict__ parent, uint64_t n, uint64_t from, uint32_t placed,
                uint32_t *__restrict__ order, uint32_t *__restrict__ ctl) {
    __shared__ uint32_t s_found;
    if (threadIdx.x == 0) s_found = kUnset;
    __syncthreads();
    for (uint64_t base = from; base < n; base += kRcmRootBlock) {  // (uniform trip count: every thread sees the same s_found)
        const uint64_t i = base + threadIdx.x;
        if (i < n && parent[by_deg[i]] == kUnset) atomicMin(&s_found, (uint32_t)i);
        __syncthreads();
        const uint32_t found = s_found;
        __syncthreads();  // (nobody offers to s_found again before everybody has read it)
        if (found != kUnset) break;
    }
    if (threadIdx.x == 0) {
        ctl[0] = 0;
        ctl[1] = s_found;
        if (s_found != kUnset) {
            const uint32_t v = by_deg[s_found];
            order[placed] = v;
            parent[v] = placed;
        }
    }
}

__device__ __forceinline__ void rcm_offer(uint32_t nb, uint32_t p, uint32_t *parent, uint32_t *cand, uint32_t *ctl) {
    if (atomicMin(&parent[nb], p) == kUnset) cand[atomicAdd(&ctl[0], 1u)] = nb;
}

__global__ void __launch_bounds__(kBlock)
k_rcm_expand(const uint32_t *__restrict__ order, uint32_t fb, uint32_t fe, const uint32_t *__restrict__ adj_off, const uint32_t *__restrict__ adj_col,
             uint32_t *__restrict__ parent, uint32_t *__restrict__ cand, uint32_t *__restrict__ ctl) {
    __shared__ uint32_t s_long[kBlock];
    __shared__ uint32_t s_nlong;
    if (threadIdx.x == 0) s_nlong = 0;
    __syncthreads();
    const uint64_t width = (uint64_t)fe - fb;
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < width; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t w = base + threadIdx.x;
        if (w < width) {
            const uint32_t p = fb + (uint32_t)w, v = order[p];
            const uint32_t b = adj_off[v], e = adj_off[v + 1];
            if (e - b <= kRcmThreadDeg) {
                for (uint32_t q = b; q < e; ++q) rcm_offer(adj_col[q], p, parent, cand, ctl);
            } else {
                s_long[atomicAdd(&s_nlong, 1u)] = p;
            }
        }
        __syncthreads();
        const uint32_t nl = s_nlong;
        for (uint32_t i = 0; i < nl; ++i) {
            const uint32_t p = s_long[i], v = order[p];
            const uint32_t e = adj_off[v + 1];
            for (uint64_t q = (uint64_t)adj_off[v] + threadIdx.x; q < e; q += kBlock) rcm_offer(adj_col[q], p, parent, cand, ctl);
        }
        __syncthreads();
        if (threadIdx.x == 0) s_nlong = 0;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kBlock)
k_rcm_level_keys(const uint32_t *__restrict__ cand, uint64_t cnt, const uint32_t *__restrict__ parent, const uint32_t *__restrict__ deg, uint32_t fb,
                 unsigned deg_bits, uint64_t *__restrict__ keys) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t v = cand[i];
        keys[i] = ((uint64_t)(parent[v] - fb) << deg_bits) | deg[v];
    }
}

__global__ void __launch_bounds__(kBlock)
k_rcm_place(const uint32_t *__restrict__ level, uint64_t cnt, uint32_t fe, uint32_t *__restrict__ order, uint32_t *__restrict__ ctl) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (uint64_t)gridDim.x * blockDim.x) order[fe + i] = level[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl[0] = 0;
}

__global__ void __launch_bounds__(kBlock)
k_rcm_reverse(const uint32_t *__restrict__ order, uint64_t n, uint32_t *__restrict__ perm) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) perm[i] = order[n - 1 - i];
}

// temporary storage of the per-level sorts: grown when a level asks for more (after the stream has drained: the level before may still use it)
struct SortTmp {
    DevArray<char> d;
    size_t cap = 0;
    int ensure(size_t bytes, hipStream_t s) {
        if (bytes <= cap) return SMH_OK;
        SMH_HIP(hipStreamSynchronize(s));
        cap = 0;
        SMH_TRY(d.alloc(bytes));
        cap = bytes;
        return SMH_OK;
    }
};

}  // namespace

// The symmetrised pattern of a square pattern of n > 0 rows whose columns are all below n (the set-up at the top of this file):
// adj_off [n + 1] / adj_col, every neighbour list ascending, both owned by scr.  The set-up arrays are gone when it returns.
int symmetrised_pattern(const uint32_t *off, const uint32_t *col, size_t n, size_t nnz, Scratch &scr, uint32_t **adj_off_out, uint32_t **adj_col_out,
                        hipStream_t s) {
    const uint64_t m2 = 2 * (uint64_t)nnz;
    if (m2 + 1 >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "the ordering handles fewer than 2^31 stored entries (%zu given)", nnz);
    uint32_t *adj_off = nullptr, *adj_col = nullptr;
    SMH_TRY(scr.alloc(&adj_off, n + 1));
    uint64_t m_u = 0;
    if (nnz) {
        Scratch setup;
        uint32_t *rows = nullptr, *pos = nullptr;
        uint64_t *keys_in = nullptr, *keys = nullptr;
        SMH_TRY(setup.alloc(&rows, nnz));
        SMH_TRY(setup.alloc(&keys_in, m2));
        SMH_TRY(setup.alloc(&keys, m2));
        SMH_TRY(expand_rows(off, n, rows, s));
        hipLaunchKernelGGL(k_rcm_keys, dim3(grid_for(nnz, kBuildGrid)), dim3(kBlock), 0, s, rows, col, (uint64_t)nnz, (uint64_t)n, keys_in);
        SMH_HIP(hipGetLastError());
        SMH_ROCPRIM(s, rocprim::radix_sort_keys(tmp, bytes, keys_in, keys, (size_t)m2, 0u, 32u + bits_for(n), s));
        setup.free_now(rows);
        setup.free_now(keys_in);
        SMH_TRY(setup.alloc(&pos, m2 + 1));
        hipLaunchKernelGGL(k_rcm_heads, dim3(grid_for(m2 + 1, kBuildGrid)), dim3(kBlock), 0, s, keys, m2, (uint64_t)n, pos);
        SMH_HIP(hipGetLastError());
        SMH_TRY(device_exclusive_scan_u32(pos, m2 + 1, s, &m_u));
        SMH_TRY(scr.alloc(&adj_col, m_u));
        hipLaunchKernelGGL(k_rcm_adj_col, dim3(grid_for(m2, kBuildGrid)), dim3(kBlock), 0, s, keys, pos, m2, (uint64_t)n, adj_col);
        SMH_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_rcm_adj_off, dim3(grid_for(n + 1, kBuildGrid)), dim3(kBlock), 0, s, keys, pos, m2, (uint64_t)n, adj_off);
        SMH_HIP(hipGetLastError());
        SMH_HIP(hipStreamSynchronize(s));  // (before the set-up arrays go)
    } else {
        SMH_TRY(scr.alloc(&adj_col, 1));
        SMH_HIP(hipMemsetAsync(adj_off, 0, (n + 1) * sizeof(uint32_t), s));
    }
    *adj_off_out = adj_off;
    *adj_col_out = adj_col;
    return SMH_OK;
}

// perm_out: device array of n entries.  off / col: a square pattern of n rows whose columns are all below n (the caller's checks).
int rcm_order(const uint32_t *off, const uint32_t *col, size_t n, size_t nnz, uint32_t *perm_out, size_t *n_components, size_t *n_levels, hipStream_t s) {
    *n_components = *n_levels = 0;
    if (n == 0) return SMH_OK;
    Scratch scr;
    uint32_t *adj_off = nullptr, *adj_col = nullptr;
    SMH_TRY(symmetrised_pattern(off, col, n, nnz, scr, &adj_off, &adj_col, s));
    // ---- degrees, the vertices by (deg, index), the isolated ones ----
    uint32_t *deg = nullptr, *iota = nullptr, *deg_sorted = nullptr, *by_deg = nullptr, *ctl = nullptr, *parent = nullptr, *order = nullptr;
    uint32_t *cand = nullptr, *cand_sorted = nullptr, *level = nullptr;
    uint64_t *lkeys = nullptr, *lkeys_sorted = nullptr;
    SMH_TRY(scr.alloc(&deg, n));
    SMH_TRY(scr.alloc(&iota, n));
    SMH_TRY(scr.alloc(&deg_sorted, n));
    SMH_TRY(scr.alloc(&by_deg, n));
    SMH_TRY(scr.alloc(&ctl, 4));
    SMH_TRY(scr.alloc(&parent, n));
    SMH_TRY(scr.alloc(&order, n));
    SMH_HIP(hipMemsetAsync(ctl, 0, 4 * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_rcm_degrees, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, adj_off, (uint64_t)n, deg, iota, ctl + 2);
    SMH_HIP(hipGetLastError());
    uint32_t h_ctl[4] = {0, 0, 0, 0};
    SMH_HIP(hipMemcpyAsync(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, s));
    SMH_HIP(hipStreamSynchronize(s));
    const size_t n_iso = h_ctl[2];
    const unsigned deg_bits = bits_for(h_ctl[3]);
    SMH_ROCPRIM(s, rocprim::radix_sort_pairs(tmp, bytes, deg, deg_sorted, iota, by_deg, n, 0u, deg_bits, s));  // stable: index order inside a degree
    scr.free_now(iota);
    scr.free_now(deg_sorted);
    SMH_HIP(hipMemsetAsync(parent, 0xFF, n * sizeof(uint32_t), s));
    SMH_HIP(hipMemsetAsync(order, 0, n * sizeof(uint32_t), s));
    if (n_iso) {
        hipLaunchKernelGGL(k_rcm_place_isolated, dim3(grid_for(n_iso, kBuildGrid)), dim3(kBlock), 0, s, by_deg, (uint64_t)n_iso, order, parent);
        SMH_HIP(hipGetLastError());
    }
    size_t placed = n_iso, comps = n_iso, levels = n_iso, root_from = n_iso;
    if (placed < n) {
        const size_t room = n - n_iso;  // no level is wider
        SMH_TRY(scr.alloc(&cand, room));
        SMH_TRY(scr.alloc(&cand_sorted, room));
        SMH_TRY(scr.alloc(&level, room));
        SMH_TRY(scr.alloc(&lkeys, room));
        SMH_TRY(scr.alloc(&lkeys_sorted, room));
    }
    SortTmp tmp;
    const unsigned v_bits = bits_for(n - 1);
    while (placed < n) {
        // a component: its root is a level of its own
        hipLaunchKernelGGL(k_rcm_find_root, dim3(1), dim3(kRcmRootBlock), 0, s, by_deg, parent, (uint64_t)n, (uint64_t)root_from, (uint32_t)placed, order, ctl);
        SMH_HIP(hipGetLastError());
        size_t fb = placed, fe = placed + 1;
        bool root_round = true;
        for (;;) {
            hipLaunchKernelGGL(k_rcm_expand, dim3(grid_for(fe - fb, kRcmExpandGrid)), dim3(kBlock), 0, s, order, (uint32_t)fb, (uint32_t)fe, adj_off, adj_col, parent,
                               cand, ctl);
            SMH_HIP(hipGetLastError());
            SMH_HIP(hipMemcpyAsync(h_ctl, ctl, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            SMH_HIP(hipStreamSynchronize(s));
            if (root_round) {
                if (h_ctl[1] == kUnset) return fail(SMH_ERR_INVALID, "ordering: no unvisited vertex left with %zu of %zu placed", placed, n);
                root_from = (size_t)h_ctl[1] + 1;
                placed = fe;  // the root
                ++comps;
                ++levels;
                root_round = false;
            }
            const size_t cnt = h_ctl[0];
            if (cnt == 0) break;  // the component is complete
            if (cnt > n - placed) return fail(SMH_ERR_INVALID, "ordering: a level of %zu vertices with %zu left", cnt, n - placed);
            size_t bytes = 0;
            SMH_HIP(rocprim::radix_sort_keys(nullptr, bytes, cand, cand_sorted, cnt, 0u, v_bits, s));
            SMH_TRY(tmp.ensure(bytes, s));
            SMH_HIP(rocprim::radix_sort_keys(tmp.d.get(), bytes, cand, cand_sorted, cnt, 0u, v_bits, s));
            hipLaunchKernelGGL(k_rcm_level_keys, dim3(grid_for(cnt, kBuildGrid)), dim3(kBlock), 0, s, cand_sorted, (uint64_t)cnt, parent, deg, (uint32_t)fb, deg_bits,
                               lkeys);
            SMH_HIP(hipGetLastError());
            const unsigned key_bits = bits_for(fe - fb - 1) + deg_bits;
            SMH_HIP(rocprim::radix_sort_pairs(nullptr, bytes, lkeys, lkeys_sorted, cand_sorted, level, cnt, 0u, key_bits, s));
            SMH_TRY(tmp.ensure(bytes, s));
            SMH_HIP(rocprim::radix_sort_pairs(tmp.d.get(), bytes, lkeys, lkeys_sorted, cand_sorted, level, cnt, 0u, key_bits, s));
            hipLaunchKernelGGL(k_rcm_place, dim3(grid_for(cnt, kBuildGrid)), dim3(kBlock), 0, s, level, (uint64_t)cnt, (uint32_t)fe, order, ctl);
            SMH_HIP(hipGetLastError());
            fb = fe;
            fe += cnt;
            placed = fe;
            ++levels;
        }
    }
    hipLaunchKernelGGL(k_rcm_reverse, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, order, (uint64_t)n, perm_out);
    SMH_HIP(hipGetLastError());
    SMH_HIP(hipStreamSynchronize(s));
    *n_components = comps;
    *n_levels = levels;
    return SMH_OK;
}

// ---- the entry points ----------------------------------------------------------------------------------------------------------
static int rcm_common(const smh_crs *m, uint32_t *perm_out, size_t *n_components_out, size_t *n_levels_out, bool on_device) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (m->n_rows != m->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    if (m->n_rows && !perm_out) return fail(SMH_ERR_INVALID, "perm_out is NULL");
    SMH_TRY(columns_within_n_cols(m, "rcm"));
    ArgStage st(on_device, m->device);
    void *d_perm = nullptr;
    SMH_TRY(st.out(perm_out, m->n_rows * sizeof(uint32_t), "perm_out", &d_perm));
    SMH_TRY(st.callers_writes_first());
    SMH_HIP(hipStreamSynchronize(m->stream));
    size_t comps = 0, levels = 0;
    SMH_TRY(rcm_order(m->d_off, m->d_col, m->n_rows, m->nnz, (uint32_t *)d_perm, &comps, &levels, m->stream));
    SMH_TRY(st.finish());
    if (n_components_out) *n_components_out = comps;
    if (n_levels_out) *n_levels_out = levels;
    return SMH_OK;
}

}  // namespace smh

using namespace smh;

extern "C" {

int smh_crs_rcm(const smh_crs *m, uint32_t *perm_out, size_t *n_components_out, size_t *n_levels_out) {
    return rcm_common(m, perm_out, n_components_out, n_levels_out, false);
}
int smh_crs_rcm_dev(const smh_crs *m, uint32_t *perm_out_dev, size_t *n_components_out, size_t *n_levels_out) {
    return rcm_common(m, perm_out_dev, n_components_out, n_levels_out, true);
}

int smh_crs_bandwidth(const smh_crs *m, uint32_t *lower_out, uint32_t *upper_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    uint32_t h[2] = {0, 0};
    if (m->n_rows && m->nnz) {
        SMH_HIP(hipStreamSynchronize(m->stream));
        Scratch scr;
        uint32_t *d = nullptr;
        SMH_TRY(scr.alloc(&d, 2));
        SMH_TRY(read_back(d, h, 2, m->stream, [&](uint32_t *q) { return launch_bandwidth(m->d_off, m->d_col, m->n_rows, q, m->stream); }));
    }
    if (lower_out) *lower_out = h[0];
    if (upper_out) *upper_out = h[1];
    return SMH_OK;
}

}  // extern "C"
