// matplan.hip -- a reusable update plan for re-assembly on a fixed pattern, gfx950: what smh_crs_apply's values-only route
// (matupdate.hip) works out on every call -- each operation's target and the stable order by target -- kept across calls, so that a
// re-assembly with new values is ONE gather-and-fold pass.
//
// The contract is apply's: every target is the left fold of its operations in stream order (add_to: acc + v, one rounding; set:
// v), from the stored value or, with from_zero, from +0.  No float atomics and no partial sums: the order of additions inside a run
// is the result.
//
// Layout (all u32; bytes per operation in DESIGN.md §4):
//   pos[n_live]       the stream positions of the kept operations, grouped by run (= target), in stream order inside a run.  An
//                     operation in front of its run's last `set` cannot reach the result and is dropped when the plan is built,
//                     so only the FIRST kept operation of a run can be a `set`;
//   off[n_runs + 1]   where each run starts in pos;
//   tgt[n_runs]       the entry of the matrix the run folds into;
//   setbits           one bit per run: its first kept operation is a `set` (the fold starts from that value, the stored one is
//                     not read).
// Runs are binned when the plan is built: the short ones (at most kPlanLongRun kept operations) come first, in pos as well, then
// the long ones; execute launches one kernel per class and skips an empty class.
//   k_plan_short  a workgroup takes 256 consecutive runs, one per thread.  Their operations are one contiguous piece of pos: the
//                 workgroup reads it with aligned 16-byte loads, issues ALL the value gathers of the piece (the only uncoalesced
//                 loads) before any add, and parks the values in LDS; then every thread folds its run from LDS in order.
//   k_plan_long   a workgroup takes one run: it stages kPlanStage operations per round in LDS (the gathers of the next round are in
//                 flight while the round is folded), and one lane folds each round from LDS in order -- serial, as the contract
//                 demands, but without a global round trip per step.
#include <new>

#include "arg_stage.hpp"
#include "crs_forms.hpp"

namespace smh {

constexpr int kPlanStage = 2048;                     // operations staged per round, both kernels
constexpr int kPlanPer = kPlanStage / kBlock;        // ... per thread: 8 (two 16-byte loads of pos)

template <typename T> __device__ __forceinline__ T plan_add(T a, T b) {  // one rounding, never contracted (matupdate.hip's upd_add)
    if constexpr (sizeof(T) == 4) return __fadd_rn(a, b);
    else return __dadd_rn(a, b);
}

// ---- execute ---------------------------------------------------------------------------------------------------------------
// pos4: pos as 16-byte chunks, n_pos4 of them (the array is padded with zeros to a whole chunk)
template <typename T, bool FROM_ZERO>
__global__ void __launch_bounds__(kBlock)
k_plan_short(const uint4 *__restrict__ pos4, uint64_t n_pos4, const uint32_t *__restrict__ off, const uint32_t *__restrict__ tgt,
             const uint32_t *__restrict__ setbits, uint64_t n_short, const T *__restrict__ values, T *val) {
    __shared__ __align__(16) T stage[kPlanStage];
    const uint64_t r0 = (uint64_t)blockIdx.x * kBlock, r = r0 + threadIdx.x;
    const uint64_t r1 = r0 + kBlock < n_short ? r0 + kBlock : n_short;
    const uint32_t tile_lo = off[r0], tile_hi = off[r1];  // the workgroup's piece of pos
    const bool mine = r < n_short;
    uint32_t s0 = tile_hi, s1 = tile_hi, t = 0;
    bool head_set = false;
    if (mine) {
        s0 = off[r];
        s1 = off[r + 1];
        t = tgt[r];
        head_set = (setbits[r >> 5] >> (r & 31)) & 1u;
    }
    T acc = T(0);
    if (!FROM_ZERO && mine && !head_set) acc = val[t];  // (in flight during the staging)
    for (uint64_t b = tile_lo & ~3u; b < tile_hi; b += kPlanStage) {
        // stage: the plan by aligned 16-byte loads, then every gather of the round, then the LDS writes
        uint4 p[kPlanPer / 4];
        T v[kPlanPer];
#pragma unroll
        for (int u = 0; u < kPlanPer / 4; ++u) {
            const uint64_t c = (b >> 2) + (uint64_t)u * kBlock + threadIdx.x;
            p[u] = (c < n_pos4 && 4 * c < tile_hi) ? pos4[c] : make_uint4(0, 0, 0, 0);  // (nothing past the piece is read)
        }
#pragma unroll
        for (int u = 0; u < kPlanPer / 4; ++u) {
            const uint64_t e = b + 4 * ((uint64_t)u * kBlock + threadIdx.x);
            const uint32_t q[4] = {p[u].x, p[u].y, p[u].z, p[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * u + j] = (e + j >= tile_lo && e + j < tile_hi) ? values[q[j]] : T(0);
        }
#pragma unroll
        for (int u = 0; u < kPlanPer / 4; ++u) {  // a chunk's four values as 16-byte LDS stores, as it was loaded
            const int c = u * kBlock + threadIdx.x;
            if constexpr (sizeof(T) == 4) {
                reinterpret_cast<float4 *>(stage)[c] = make_float4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
            } else {
                reinterpret_cast<double2 *>(stage)[2 * c] = make_double2(v[4 * u], v[4 * u + 1]);
                reinterpret_cast<double2 *>(stage)[2 * c + 1] = make_double2(v[4 * u + 2], v[4 * u + 3]);
            }
        }
        __syncthreads();
        // fold the part of this thread's run that the round holds
        const uint64_t lo = s0 > b ? s0 : b, hi = s1 < b + kPlanStage ? s1 : b + kPlanStage;
        for (uint64_t e = lo; e < hi; ++e) {
            const T x = stage[e - b];
            acc = (head_set && e == s0) ? x : plan_add(acc, x);
        }
        __syncthreads();
    }
    if (mine) val[t] = acc;
}

// runs [r_begin, r_end): one workgroup per run, grid-stride
template <typename T, bool FROM_ZERO>
__global__ void __launch_bounds__(kBlock)
k_plan_long(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ off, const uint32_t *__restrict__ tgt,
            const uint32_t *__restrict__ setbits, uint64_t r_begin, uint64_t r_end, const T *__restrict__ values, T *val) {
    __shared__ T stage[kPlanStage];
    for (uint64_t r = r_begin + blockIdx.x; r < r_end; r += gridDim.x) {
        const uint32_t s0 = off[r], s1 = off[r + 1], t = tgt[r];
        const bool head_set = (setbits[r >> 5] >> (r & 31)) & 1u;
        T acc = T(0);
        if (!FROM_ZERO && !head_set && threadIdx.x == 0) acc = val[t];
        T v[kPlanPer];
        auto gather = [&](uint64_t b) {  // the round's positions by coalesced loads, then its gathers
            uint32_t q[kPlanPer];
#pragma unroll
            for (int u = 0; u < kPlanPer; ++u) {
                const uint64_t e = b + (uint64_t)u * kBlock + threadIdx.x;
                q[u] = e < s1 ? pos[e] : 0u;
            }
#pragma unroll
            for (int u = 0; u < kPlanPer; ++u) {
                const uint64_t e = b + (uint64_t)u * kBlock + threadIdx.x;
                v[u] = e < s1 ? values[q[u]] : T(0);
            }
        };
        gather(s0);
        for (uint64_t b = s0; b < s1; b += kPlanStage) {
#pragma unroll
            for (int u = 0; u < kPlanPer; ++u) stage[u * kBlock + threadIdx.x] = v[u];
            __syncthreads();
            if (b + kPlanStage < s1) gather(b + kPlanStage);  // in flight while lane 0 folds
            if (threadIdx.x == 0) {
                const uint32_t cnt = s1 - b < (uint64_t)kPlanStage ? (uint32_t)(s1 - b) : (uint32_t)kPlanStage;
                uint32_t j = 0;
                if (head_set && b == s0) {
                    acc = stage[0];
                    j = 1;
                }
#pragma unroll 8
                for (; j < cnt; ++j) acc = plan_add(acc, stage[j]);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) val[t] = acc;
    }
}

template <typename T, bool FROM_ZERO>
static int execute_t(const UpdPlan &p, const T *values, T *m_val, hipStream_t s) {
    if (p.n_short) {
        const uint64_t n_pos4 = (p.n_live + 3) / 4;
        const uint64_t blocks = (p.n_short + kBlock - 1) / kBlock;
        hipLaunchKernelGGL((k_plan_short<T, FROM_ZERO>), dim3((unsigned)blocks), dim3(kBlock), 0, s, (const uint4 *)p.pos.get(), n_pos4,
                           (const uint32_t *)p.off.get(), (const uint32_t *)p.tgt.get(), (const uint32_t *)p.setbits.get(), (uint64_t)p.n_short, values,
                           m_val);
        SMH_HIP(hipGetLastError());
    }
    if (p.n_targets > p.n_short) {
        const uint64_t n_long = p.n_targets - p.n_short;
        hipLaunchKernelGGL((k_plan_long<T, FROM_ZERO>), dim3((unsigned)(n_long < kBuildGrid ? n_long : kBuildGrid)), dim3(kBlock), 0, s,
                           (const uint32_t *)p.pos.get(), (const uint32_t *)p.off.get(), (const uint32_t *)p.tgt.get(), (const uint32_t *)p.setbits.get(),
                           (uint64_t)p.n_short, (uint64_t)p.n_targets, values, m_val);
        SMH_HIP(hipGetLastError());
    }
    return SMH_OK;
}

int plan_execute(int dtype, const UpdPlan &p, const void *values, void *m_val, bool from_zero, hipStream_t s) {
    if (dtype == SMH_F64)
        return from_zero ? execute_t<double, true>(p, (const double *)values, (double *)m_val, s)
                         : execute_t<double, false>(p, (const double *)values, (double *)m_val, s);
    return from_zero ? execute_t<float, true>(p, (const float *)values, (float *)m_val, s)
                     : execute_t<float, false>(p, (const float *)values, (float *)m_val, s);
}

// ---- build -----------------------------------------------------------------------------------------------------------------
// key / src: the operations in (target, stream order).  q is a position in that order, r a run in target order.
// flag[q] = 1 at the head of a run, flag[n] = 0 (the caller scans the flags: run of q = scanned[q + 1] - 1)
__global__ void __launch_bounds__(kBlock) k_plan_head_flags(const uint32_t *__restrict__ key, uint64_t n, uint32_t *__restrict__ flag) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= n; q += (uint64_t)gridDim.x * blockDim.x)
        flag[q] = (q < n && (q == 0 || key[q - 1] != key[q])) ? 1u : 0u;
}

// begin[r] = first q of run r (begin[n_runs] = n), rkey[r] = its target, last_set[r] = 1 + the last q of the run that is a `set`
// (0: none; integer maxima, exact whatever the order)
__global__ void __launch_bounds__(kBlock)
k_plan_runs(const uint32_t *__restrict__ key, const uint32_t *__restrict__ src, const uint8_t *__restrict__ ops, uint64_t n,
            const uint32_t *__restrict__ hpos, uint32_t *__restrict__ begin, uint32_t *__restrict__ rkey, uint32_t *__restrict__ last_set) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= n; q += (uint64_t)gridDim.x * blockDim.x) {
        if (q == n) {
            begin[hpos[n]] = (uint32_t)n;
            continue;
        }
        const uint32_t r = hpos[q + 1] - 1;
        if (hpos[q] != hpos[q + 1]) {
            begin[r] = (uint32_t)q;
            rkey[r] = key[q];
        }
        if (ops && ops[src[q]]) atomicMax(&last_set[r], (uint32_t)q + 1);
    }
}

// per run: its first kept operation and kept length; len_s / len_l, cnt_s / cnt_l (n_runs + 1 each, the last zero) are what the
// caller scans to place the short runs in front of the long ones; *longest = most operations on one target, dropped ones included
__global__ void __launch_bounds__(kBlock)
k_plan_lengths(const uint32_t *__restrict__ begin, const uint32_t *__restrict__ last_set, uint64_t n_runs, uint32_t *__restrict__ first,
               uint32_t *__restrict__ len_s, uint32_t *__restrict__ len_l, uint32_t *__restrict__ cnt_s, uint32_t *__restrict__ cnt_l,
               uint32_t *__restrict__ longest) {
    uint32_t most = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_runs; r += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t len = 0, f = 0;
        if (r < n_runs) {
            const uint32_t b = begin[r], e = begin[r + 1], ls = last_set[r];
            f = ls ? ls - 1 : b;
            len = e - f;
            most = e - b > most ? e - b : most;
        }
        const bool is_long = len > kPlanLongRun;
        first[r] = f;
        len_s[r] = is_long ? 0u : len;
        len_l[r] = is_long ? len : 0u;
        cnt_s[r] = (r < n_runs && !is_long) ? 1u : 0u;
        cnt_l[r] = is_long ? 1u : 0u;
    }
    most = wave_max_u32(most);
    if ((threadIdx.x & (kWave - 1)) == 0) atomicMax(longest, most);
}

// the run descriptors in class order; len_s[r] becomes where run r starts in pos
__global__ void __launch_bounds__(kBlock)
k_plan_descriptors(const uint32_t *__restrict__ begin, const uint32_t *__restrict__ first, const uint32_t *__restrict__ rkey,
                   const uint32_t *__restrict__ last_set, uint64_t n_runs, uint32_t *__restrict__ len_s, const uint32_t *__restrict__ len_l,
                   const uint32_t *__restrict__ cnt_s, const uint32_t *__restrict__ cnt_l, uint32_t n_short, uint32_t live_short, uint32_t n_live,
                   uint32_t *__restrict__ off, uint32_t *__restrict__ tgt, uint32_t *__restrict__ setbits) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_runs; r += (uint64_t)gridDim.x * blockDim.x) {
        const bool is_long = begin[r + 1] - first[r] > kPlanLongRun;
        const uint32_t i = is_long ? n_short + cnt_l[r] : cnt_s[r];
        const uint32_t start = is_long ? live_short + len_l[r] : len_s[r];
        off[i] = start;
        tgt[i] = rkey[r];
        if (last_set[r]) atomicOr(&setbits[i >> 5], 1u << (i & 31));
        len_s[r] = start;
        if (r == 0) off[n_runs] = n_live;
    }
}

__global__ void __launch_bounds__(kBlock)
k_plan_positions(const uint32_t *__restrict__ src, uint64_t n, const uint32_t *__restrict__ hpos, const uint32_t *__restrict__ first,
                 const uint32_t *__restrict__ start, uint32_t *__restrict__ pos) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = hpos[q + 1] - 1, f = first[r];
        if (q >= f) pos[start[r] + ((uint32_t)q - f)] = src[q];
    }
}

int plan_build(size_t n, const uint32_t *key, const uint32_t *src, const uint8_t *ops, UpdPlan *plan, hipStream_t s) {
    Scratch scr;
    uint32_t *hpos = nullptr;
    uint64_t n_runs = 0;
    SMH_TRY(scr.alloc(&hpos, n + 1));
    hipLaunchKernelGGL(k_plan_head_flags, dim3(grid_for(n + 1, kBuildGrid)), dim3(kBlock), 0, s, key, (uint64_t)n, hpos);
    SMH_HIP(hipGetLastError());
    SMH_TRY(device_exclusive_scan_u32(hpos, n + 1, s, &n_runs));
    uint32_t *begin = nullptr, *rkey = nullptr, *last_set = nullptr, *first = nullptr, *len_s = nullptr, *len_l = nullptr, *cnt_s = nullptr,
             *cnt_l = nullptr, *longest = nullptr;
    SMH_TRY(scr.alloc(&begin, n_runs + 1));
    SMH_TRY(scr.alloc(&rkey, n_runs));
    SMH_TRY(scr.alloc(&last_set, n_runs));
    SMH_TRY(scr.alloc(&first, n_runs + 1));
    SMH_TRY(scr.alloc(&len_s, n_runs + 1));
    SMH_TRY(scr.alloc(&len_l, n_runs + 1));
    SMH_TRY(scr.alloc(&cnt_s, n_runs + 1));
    SMH_TRY(scr.alloc(&cnt_l, n_runs + 1));
    SMH_TRY(scr.alloc(&longest, 1));
    SMH_HIP(hipMemsetAsync(last_set, 0, (n_runs ? n_runs : 1) * sizeof(uint32_t), s));
    SMH_HIP(hipMemsetAsync(longest, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_plan_runs, dim3(grid_for(n + 1, kBuildGrid)), dim3(kBlock), 0, s, key, src, ops, (uint64_t)n, (const uint32_t *)hpos, begin, rkey,
                       last_set);
    SMH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_plan_lengths, dim3(grid_for(n_runs + 1, kBuildGrid)), dim3(kBlock), 0, s, (const uint32_t *)begin, (const uint32_t *)last_set, n_runs,
                       first, len_s, len_l, cnt_s, cnt_l, longest);
    SMH_HIP(hipGetLastError());
    uint64_t live_short = 0, live_long = 0, n_short = 0, n_long = 0;
    SMH_TRY(device_exclusive_scan_u32(len_s, n_runs + 1, s, &live_short));
    SMH_TRY(device_exclusive_scan_u32(len_l, n_runs + 1, s, &live_long));
    SMH_TRY(device_exclusive_scan_u32(cnt_s, n_runs + 1, s, &n_short));
    SMH_TRY(device_exclusive_scan_u32(cnt_l, n_runs + 1, s, &n_long));
    if (n_short + n_long != n_runs) return fail(SMH_ERR_HIP, "update plan: run counts disagree");
    uint32_t h_longest = 0;
    SMH_HIP(hipMemcpyAsync(&h_longest, longest, sizeof h_longest, hipMemcpyDeviceToHost, s));
    SMH_HIP(hipStreamSynchronize(s));
    const uint64_t n_live = live_short + live_long, n_pos = (n_live + 3) / 4 * 4, n_bits = (n_runs + 31) / 32;
    UpdPlan p;
    SMH_TRY(p.pos.alloc(n_pos ? n_pos : 4));
    SMH_TRY(p.off.alloc(n_runs + 1));
    SMH_TRY(p.tgt.alloc(n_runs ? n_runs : 1));
    SMH_TRY(p.setbits.alloc(n_bits ? n_bits : 1));
    SMH_HIP(hipMemsetAsync(p.pos.get(), 0, (n_pos ? n_pos : 4) * sizeof(uint32_t), s));
    SMH_HIP(hipMemsetAsync(p.setbits.get(), 0, (n_bits ? n_bits : 1) * sizeof(uint32_t), s));
    SMH_HIP(hipMemsetAsync(p.off.get(), 0, sizeof(uint32_t), s));  // (a plan without runs: off[0] = 0)
    if (n_runs) {
        hipLaunchKernelGGL(k_plan_descriptors, dim3(grid_for(n_runs, kBuildGrid)), dim3(kBlock), 0, s, (const uint32_t *)begin, (const uint32_t *)first,
                           (const uint32_t *)rkey, (const uint32_t *)last_set, n_runs, len_s, (const uint32_t *)len_l, (const uint32_t *)cnt_s,
                           (const uint32_t *)cnt_l, (uint32_t)n_short, (uint32_t)live_short, (uint32_t)n_live, p.off.get(), p.tgt.get(), p.setbits.get());
        SMH_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_plan_positions, dim3(grid_for(n, kBuildGrid)), dim3(kBlock), 0, s, src, (uint64_t)n, (const uint32_t *)hpos, (const uint32_t *)first,
                           (const uint32_t *)len_s, p.pos.get());
        SMH_HIP(hipGetLastError());
    }
    SMH_HIP(hipStreamSynchronize(s));
    p.n_ops = n;
    p.n_targets = n_runs;
    p.n_live = n_live;
    p.longest_run = h_longest;
    p.n_short = n_short;
    p.device_bytes = ((n_pos ? n_pos : 4) + (n_runs + 1) + (n_runs ? n_runs : 1) + (n_bits ? n_bits : 1)) * sizeof(uint32_t);
    *plan = std::move(p);
    return SMH_OK;
}

}  // namespace smh

// ---- the entry points ----------------------------------------------------------------------------------------------------------
using namespace smh;

struct smh_update_plan {
    uint64_t crs_id = 0, epoch = 0;  // the handle and the structure it was made for
    UpdPlan plan;
    StageBuf stage;  // the host form's upload of the values (lazy, reused)
};

static int plan_create_common(const smh_crs *m, size_t n, const uint32_t *rows, const uint32_t *cols, const uint8_t *ops, bool on_device,
                              smh_update_plan **out) {
    if (!out) return fail(SMH_ERR_INVALID, "NULL out pointer");
    *out = nullptr;
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (n && (!rows || !cols)) return fail(SMH_ERR_INVALID, "NULL operation array");
    if (n >= 0xFFFFFFFFull) return fail(SMH_ERR_CAPACITY, "Maximum number of %u entries reached", 0xFFFFFFFFu);
    if (m->n_rows == 0) return fail(SMH_ERR_INVALID, "update plan: the handle has no rows, so no operation has an entry to land on");
    smh_update_plan *p = new (std::nothrow) smh_update_plan();
    if (!p) return fail(SMH_ERR_OOM, "host allocation failed");
    p->crs_id = m->id; p->epoch = m->epoch;
    const int rc = [&]() -> int {
        if (n == 0) return SMH_OK;  // a valid plan whose execute does nothing
        ArgStage st(on_device, m->device);  // (its scratch also holds the sorted operations)
        const void *d_rows = nullptr, *d_cols = nullptr, *d_ops = nullptr;
        SMH_TRY(st.in(rows, n * sizeof(uint32_t), "rows", &d_rows));
        SMH_TRY(st.in(cols, n * sizeof(uint32_t), "cols", &d_cols));
        SMH_TRY(st.in(ops, n, "ops", &d_ops));
        SMH_TRY(st.callers_writes_first());
        SMH_HIP(hipStreamSynchronize(m->stream));
        uint32_t *key = nullptr, *src = nullptr;
        uint64_t n_absent = 0;
        SMH_TRY(st.scratch().alloc(&key, n));
        SMH_TRY(st.scratch().alloc(&src, n));
        SMH_TRY(crs_plan_targets(upd_view(m), n, (const uint32_t *)d_rows, (const uint32_t *)d_cols, key, src, &n_absent, m->stream));
        if (n_absent)
            return fail(SMH_ERR_INVALID, "update plan: %llu of %llu operations have no entry to land on (smh_crs_apply creates entries; plan afterwards)",
                        (unsigned long long)n_absent, (unsigned long long)n);
        return plan_build(n, key, src, (const uint8_t *)d_ops, &p->plan, m->stream);
    }();
    if (rc != SMH_OK) return keep_error(rc, [&] { delete p; });
    *out = p;
    return SMH_OK;
}

static int plan_execute_common(smh_update_plan *p, smh_crs *m, const void *values, int from_zero, bool on_device) {
    if (!p || !m) return fail(SMH_ERR_INVALID, "NULL argument");
    if (p->crs_id != m->id) return fail(SMH_ERR_INVALID, "update plan: made for another handle");
    if (p->epoch != m->epoch) return fail(SMH_ERR_INVALID, "update plan: the handle's structure changed since the plan was made");
    const size_t n = p->plan.n_ops;
    if (n && !values) return fail(SMH_ERR_INVALID, "NULL value array");
    if (n == 0) return SMH_OK;
    ArgStage st(on_device, m->device);
    const void *d_vals = values;
    SMH_TRY(st.check(values, "values"));
    SMH_TRY(st.callers_writes_first());
    if (!on_device) {  // known difference, kept: the plan's own reusable staging buffer, so that repeated executes do not allocate
        const size_t bytes = n * dtype_size(m->dtype);
        SMH_TRY(p->stage.ensure_cap(bytes));
        SMH_HIP(hipMemcpy(p->stage.d.get(), values, bytes, hipMemcpyHostToDevice));
        d_vals = p->stage.d.get();
    }
    SMH_HIP(hipStreamSynchronize(m->stream));
    SMH_TRY(plan_execute(m->dtype, p->plan, d_vals, m->d_val, from_zero != 0, m->stream));
    SMH_HIP(hipStreamSynchronize(m->stream));
    return smh_crs_update_values(m, nullptr);  // as apply's values-only route: structure-derived forms stay, value-derived ones follow
}

extern "C" {

int smh_update_plan_create(const smh_crs *m, size_t n_ops, const uint32_t *rows, const uint32_t *cols, const uint8_t *ops, smh_update_plan **out) {
    return plan_create_common(m, n_ops, rows, cols, ops, false, out);
}
int smh_update_plan_create_dev(const smh_crs *m, size_t n_ops, const uint32_t *rows_dev, const uint32_t *cols_dev, const uint8_t *ops_dev,
                               smh_update_plan **out) {
    return plan_create_common(m, n_ops, rows_dev, cols_dev, ops_dev, true, out);
}

int smh_update_plan_execute(smh_update_plan *p, smh_crs *m, const void *values, int from_zero) {
    return plan_execute_common(p, m, values, from_zero, false);
}
int smh_update_plan_execute_dev(smh_update_plan *p, smh_crs *m, const void *values_dev, int from_zero) {
    return plan_execute_common(p, m, values_dev, from_zero, true);
}

int smh_update_plan_stats(const smh_update_plan *p, size_t *n_ops, size_t *n_targets, size_t *n_live_ops, size_t *longest_run,
                          size_t *long_run_threshold, size_t *device_bytes) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL plan");
    if (n_ops) *n_ops = p->plan.n_ops;
    if (n_targets) *n_targets = p->plan.n_targets;
    if (n_live_ops) *n_live_ops = p->plan.n_live;
    if (longest_run) *longest_run = p->plan.longest_run;
    if (long_run_threshold) *long_run_threshold = kPlanLongRun;
    if (device_bytes) *device_bytes = p->plan.device_bytes;
    return SMH_OK;
}

int smh_update_plan_destroy(smh_update_plan *p) {
    delete p;
    return SMH_OK;
}

}  // extern "C"
