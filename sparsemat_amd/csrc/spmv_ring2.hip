// spmv_ring2.hip -- K1r, software-pipelined body (same plan, same result as spmv_ring.hip): the instantiations of the three-body and
// REGK forms of the kernel in spmv_ring2_kernel.hpp, their launches, and the builders of the forms the ring phases stream.
#include "spmv_ring2_kernel.hpp"

#include <atomic>
#include <type_traits>

namespace smh {

// the <= 3 entries of an unpadded array's last partial chunk, appended to their rows in storage order
template <typename T>
__global__ void k_ring2_tail(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col,
                             const T *__restrict__ val, const T *__restrict__ x, T *__restrict__ y, uint64_t n_rows,
                             uint64_t k_begin, uint64_t nnz) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t r = n_rows - 1;
    while (r > 0 && (uint64_t)off[r] > k_begin) --r;  // row holding entry k_begin
    for (uint64_t k = k_begin; k < nnz; ++k) {
        while ((uint64_t)off[r + 1] <= k) ++r;
        y[r] = r2_fma(val[k], x[col[k]], y[r]);
    }
}

// ... and for the DOT form: *out = sum over those entries of lhs[row] * val * x[col] (their share of lhs . (A x))
template <typename T>
__global__ void k_ring2_tail_dot(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val,
                                 const T *__restrict__ x, const T *__restrict__ lhs, T *__restrict__ out, uint64_t n_rows, uint64_t k_begin,
                                 uint64_t nnz) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t r = n_rows - 1;
    while (r > 0 && (uint64_t)off[r] > k_begin) --r;
    T acc = T(0);
    for (uint64_t k = k_begin; k < nnz; ++k) {
        while ((uint64_t)off[r + 1] <= k) ++r;
        acc = r2_fma(lhs[r], val[k] * x[col[k]], acc);
    }
    *out = acc;
}

// col16[k] = low half of col[k] (k < nnz), zero padding up to the next multiple of 4 entries and one chunk beyond
__global__ void __launch_bounds__(kBlock)
k_narrow_columns(const uint32_t *__restrict__ col, uint64_t nnz, uint64_t n_out, uint16_t *__restrict__ col16) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_out; k += (uint64_t)gridDim.x * blockDim.x)
        col16[k] = k < nnz ? (uint16_t)col[k] : (uint16_t)0;
}

int launch_narrow_columns(const uint32_t *col, size_t nnz, uint16_t *col16, size_t n_out, hipStream_t s) {
    if (n_out == 0) return SMH_OK;
    uint64_t blocks = (n_out + kBlock - 1) / kBlock;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_narrow_columns, dim3((unsigned)blocks), dim3(kBlock), 0, s, col, (uint64_t)nnz, (uint64_t)n_out, col16);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// ---- which ring phases are regular (RingPlan::reg_len), once per plan ----
// One workgroup per phase at a time: L = the first row's length, and every offset of rows [row_begin, row_end] is compared with
// off[row_begin] + (r - row_begin) * L (in 64 bits: a product that wraps must not pass).  Each offset is read once, except those
// two phases share.
__global__ void __launch_bounds__(kBlock)
k_ring_regular(const uint32_t *__restrict__ off, const RingPhase *__restrict__ phases, uint32_t n_phases, uint32_t *__restrict__ reg_len) {
    __shared__ uint32_t s_bad;
    for (uint32_t p = blockIdx.x; p < n_phases; p += gridDim.x) {
        const uint32_t rb = phases[p].row_begin, re = phases[p].row_end;
        const bool ring = phases[p].use_ring == 1u && re > rb;
        if (threadIdx.x == 0) s_bad = 0u;
        __syncthreads();
        uint32_t L = 0;
        if (ring) {  // (workgroup-uniform)
            const uint32_t e0 = off[rb];
            L = off[rb + 1] - e0;
            bool bad = false;
            for (uint64_t r = (uint64_t)rb + threadIdx.x; r <= re; r += kBlock) bad |= (uint64_t)off[r] != (uint64_t)e0 + (r - rb) * (uint64_t)L;
            if (bad) s_bad = 1u;
        }
        __syncthreads();
        if (threadIdx.x == 0) reg_len[p] = s_bad ? 0u : L;
        __syncthreads();  // (s_bad is read before the next phase clears it)
    }
}

int launch_ring_regular(const uint32_t *off, const RingPhase *phases, size_t n_phases, uint32_t *reg_len, hipStream_t s) {
    if (n_phases == 0) return SMH_OK;
    hipLaunchKernelGGL(k_ring_regular, dim3((unsigned)(n_phases < 8192 ? n_phases : 8192)), dim3(kBlock), 0, s, off, phases, (uint32_t)n_phases,
                       reg_len);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// ---- the compact column form (ring_col12.hpp), built once per matrix ----
// Which chunks the ring phases stream: jobs[p] = chunks [x, y) of phase p (empty for a global-gather phase), every chunk in
// one job only -- a chunk that two ring phases share (a phase begins inside it) goes with the earlier one.  Phases follow
// one another in row order, so the entry before phase p's first belongs to the nearest earlier phase that has entries.
__global__ void __launch_bounds__(kBlock)
k_col12_jobs(const uint32_t *__restrict__ off, const RingPhase *__restrict__ phases, uint32_t n_phases, u32x2 *__restrict__ jobs,
             unsigned long long *__restrict__ counts) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_phases) return;
    const uint32_t e0 = off[phases[p].row_begin], e1 = off[phases[p].row_end];
    uint32_t cb = e0 >> 2, ce = (uint32_t)(((uint64_t)e1 + 3u) >> 2);
    if (phases[p].use_ring != 1u || e1 <= e0) {
        cb = ce = 0;
    } else if (e0 & 3u) {
        uint32_t q = p;
        while (q > 0 && off[phases[q - 1].row_begin] == e0) --q;  // (earlier phases without entries)
        if (q > 0 && phases[q - 1].use_ring == 1u) ++cb;
    }
    jobs[p] = u32x2{cb, ce > cb ? ce : cb};
    if (ce > cb) atomicAdd(&counts[0], (unsigned long long)(ce - cb));
}

// COUNT: counts[1] += the jobs' chunks the code cannot hold.  Else: the jobs' chunks are encoded; an escaped one takes the
// next free entry of the side table (counts[1] is the allocator, from 0), so the table's order differs from run to run --
// the slots a chunk decodes to do not.  Columns past nnz count as 0, like col16's padding.
template <bool COUNT>
__global__ void __launch_bounds__(kBlock)
k_col12_encode(const uint32_t *__restrict__ col, uint64_t nnz, const u32x2 *__restrict__ jobs, uint32_t n_jobs, uint32_t *__restrict__ lo,
               uint16_t *__restrict__ hdr, u32x2 *__restrict__ escapes, unsigned long long *__restrict__ counts) {
    unsigned long long mine = 0;
    for (uint32_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const u32x2 range = jobs[job];
        for (uint64_t c = (uint64_t)range.x + threadIdx.x; c < range.y; c += kBlock) {
            uint32_t slot[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) slot[q] = (4u * c + q < nnz ? col[4u * c + q] : 0u) & (col12::kSlots - 1u);
            uint16_t h = 0;
            uint32_t l = 0;
            const bool ok = col12::encode_chunk(slot, &h, &l);
            if constexpr (COUNT) {
                mine += ok ? 0u : 1u;
            } else {
                if (!ok) {
                    l = (uint32_t)atomicAdd(&counts[1], 1ull);
                    h = (uint16_t)col12::kEscape;
                    uint32_t pair[2];
                    col12::pack_escape(slot, pair);
                    escapes[l] = u32x2{pair[0], pair[1]};
                }
                lo[c] = l;
                hdr[c] = h;
            }
        }
    }
    if constexpr (COUNT) {
        if (mine) atomicAdd(&counts[1], mine);
    }
}

int launch_col12_count(const uint32_t *off, const uint32_t *col, size_t nnz, const RingPhase *phases, size_t n_phases, uint32_t *jobs,
                       unsigned long long *counts, hipStream_t s) {
    SMH_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), s));
    if (n_phases == 0) return SMH_OK;
    hipLaunchKernelGGL(k_col12_jobs, dim3((unsigned)((n_phases + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, off, phases, (uint32_t)n_phases,
                       reinterpret_cast<u32x2 *>(jobs), counts);
    SMH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_col12_encode<true>, dim3((unsigned)(n_phases < 8192 ? n_phases : 8192)), dim3(kBlock), 0, s, col, (uint64_t)nnz,
                       reinterpret_cast<const u32x2 *>(jobs), (uint32_t)n_phases, (uint32_t *)nullptr, (uint16_t *)nullptr, (u32x2 *)nullptr, counts);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

int launch_col12_encode(const uint32_t *col, size_t nnz, const uint32_t *jobs, size_t n_phases, size_t n_chunks_out, uint8_t *lo8,
                        uint16_t *hdr, uint32_t *escapes, unsigned long long *counts, hipStream_t s) {
    // chunks no ring phase streams, and the padding: header 0 -- they decode to slots inside the ring like any other
    SMH_HIP(hipMemsetAsync(lo8, 0, n_chunks_out * 4, s));
    SMH_HIP(hipMemsetAsync(hdr, 0, n_chunks_out * sizeof(uint16_t), s));
    SMH_HIP(hipMemsetAsync(counts + 1, 0, sizeof(unsigned long long), s));
    if (n_phases == 0) return SMH_OK;
    hipLaunchKernelGGL(k_col12_encode<false>, dim3((unsigned)(n_phases < 8192 ? n_phases : 8192)), dim3(kBlock), 0, s, col, (uint64_t)nnz,
                       reinterpret_cast<const u32x2 *>(jobs), (uint32_t)n_phases, reinterpret_cast<uint32_t *>(lo8), hdr,
                       reinterpret_cast<u32x2 *>(escapes), counts);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// ---- the chunk records of the 24-bit value code (ring_val24.hpp), built once per matrix and set of values ----
// The values of a chunk (entries past nnz count as +0, like the padding of an owned array)
__device__ __forceinline__ void val24_chunk_values(const float *__restrict__ val, uint64_t nnz, uint64_t c, float (&v)[4]) {
    if (4u * c + 3u < nnz) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(val + 4u * c);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = 4u * c + q < nnz ? val[4u * c + q] : 0.0f;
    }
}

// The counting pass over the jobs' chunks (k_col12_jobs): stats[0] = min over the non-zero values of 1024 + the exponent of the
// value's lowest set mantissa bit (from ~0u) -- the largest E all of them are multiples of 2^E for; stats[1] != 0: some value is
// NaN, +-Inf, -0.0 or subnormal
__global__ void __launch_bounds__(kBlock)
k_val24_count(const float *__restrict__ val, uint64_t nnz, const u32x2 *__restrict__ jobs, uint32_t n_jobs, uint32_t *__restrict__ stats) {
    uint32_t lowest = ~0u, bad = 0u;
    for (uint32_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const u32x2 range = jobs[job];
        for (uint64_t c = (uint64_t)range.x + threadIdx.x; c < range.y; c += kBlock) {
            float v[4];
            val24_chunk_values(val, nnz, c, v);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t bits = val24::float_bits(v[q]);
                if (val24::never_fits(bits)) bad = 1u;
                else if (bits != 0u) {
                    const uint32_t e = (uint32_t)(1024 + val24::lowest_bit_exponent(bits));
                    lowest = e < lowest ? e : lowest;
                }
            }
        }
    }
    if (lowest != ~0u) atomicMin(&stats[0], lowest);
    if (bad) atomicOr(&stats[1], 1u);
}

// The records of the jobs' chunks: {three dwords of 24-bit integers, the chunk's dword of lo8}.  *misses += the values that do not
// come back bit for bit from what was written for them (they are written as 0): the form is only taken when there is none.
__global__ void __launch_bounds__(kBlock)
k_val24_encode(const float *__restrict__ val, uint64_t nnz, const u32x2 *__restrict__ jobs, uint32_t n_jobs, const uint32_t *__restrict__ lo,
               int E, u32x4 *__restrict__ rec, unsigned long long *__restrict__ misses) {
    unsigned long long mine = 0;
    for (uint32_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const u32x2 range = jobs[job];
        for (uint64_t c = (uint64_t)range.x + threadIdx.x; c < range.y; c += kBlock) {
            float v[4];
            val24_chunk_values(val, nnz, c, v);
            int32_t k[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                k[q] = 0;
                if (!val24::encode(v[q], E, &k[q])) ++mine;
            }
            uint32_t w[3];
            val24::pack(k, w);
            rec[c] = u32x4{w[0], w[1], w[2], lo[c]};
        }
    }
    if (mine) atomicAdd(misses, mine);
}

int launch_val24_count(const uint32_t *off, const float *val, size_t nnz, const RingPhase *phases, size_t n_phases, uint32_t *jobs,
                       unsigned long long *counts, uint32_t *stats, hipStream_t s) {
    SMH_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), s));
    SMH_HIP(hipMemsetAsync(stats, 0xFF, sizeof(uint32_t), s));
    SMH_HIP(hipMemsetAsync(stats + 1, 0, sizeof(uint32_t), s));
    if (n_phases == 0) return SMH_OK;
    hipLaunchKernelGGL(k_col12_jobs, dim3((unsigned)((n_phases + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, off, phases, (uint32_t)n_phases,
                       reinterpret_cast<u32x2 *>(jobs), counts);
    SMH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_val24_count, dim3((unsigned)(n_phases < 8192 ? n_phases : 8192)), dim3(kBlock), 0, s, val, (uint64_t)nnz,
                       reinterpret_cast<const u32x2 *>(jobs), (uint32_t)n_phases, stats);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

int launch_val24_encode(const float *val, size_t nnz, const uint32_t *jobs, size_t n_phases, size_t n_chunks_out, const uint8_t *lo8, int exponent,
                        uint32_t *rec16, unsigned long long *misses, hipStream_t s) {
    // chunks no ring phase streams, and the padding: all zero, i.e. four values +0 over the low bytes lo8 has there
    SMH_HIP(hipMemsetAsync(rec16, 0, n_chunks_out * 16, s));
    SMH_HIP(hipMemsetAsync(misses, 0, sizeof(unsigned long long), s));
    if (n_phases == 0) return SMH_OK;
    hipLaunchKernelGGL(k_val24_encode, dim3((unsigned)(n_phases < 8192 ? n_phases : 8192)), dim3(kBlock), 0, s, val, (uint64_t)nnz,
                       reinterpret_cast<const u32x2 *>(jobs), (uint32_t)n_phases, reinterpret_cast<const uint32_t *>(lo8), exponent,
                       reinterpret_cast<u32x4 *>(rec16), misses);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// k_ring2_tail behind a product's launch that covers the last rows (every form of the kernel: spmv_ring2_allreg.hip calls it too)
int launch_ring2_tail(int dtype, const uint32_t *off, const uint32_t *col, const void *val, const void *x, void *y, size_t n_rows,
                      uint64_t k_begin, size_t nnz, hipStream_t s) {
    if (dtype == SMH_F64)
        hipLaunchKernelGGL(k_ring2_tail<double>, dim3(1), dim3(64), 0, s, off, col, (const double *)val, (const double *)x, (double *)y,
                           (uint64_t)n_rows, k_begin, (uint64_t)nnz);
    else
        hipLaunchKernelGGL(k_ring2_tail<float>, dim3(1), dim3(64), 0, s, off, col, (const float *)val, (const float *)x, (float *)y,
                           (uint64_t)n_rows, k_begin, (uint64_t)nnz);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// dot_partials != NULL: the DOT form -- `y` is lhs (read only), dot_partials[0..n_blocks] receive the blocks' shares of
// lhs . (A x) plus, in slot n_blocks, that of an unpadded array's last partial chunk
// resident_out != NULL: a query, nothing is enqueued -- *resident_out = how many workgroups of the kernel this call would launch a CU
// holds at once (with its dynamic LDS; 0: it would launch none), *threads_out their size
template <typename T, int RING>
static int launch_ring2_t(int lanes, int chunks, const uint32_t *off, const uint32_t *col, const uint16_t *col16, const RingCol12 &c12, const T *val,
                          const T *x, T *y, size_t n_rows, size_t nnz, bool padded, unsigned n_blocks,
                          const uint32_t *phase_ptr, const RingPhase *phases, uint32_t bands, T *dot_partials, hipStream_t s,
                          unsigned block_begin, unsigned block_end, const uint32_t *reg_len, int *resident_out, int *threads_out) {
    if (bands == 4u && !col16) return fail(SMH_ERR_INVALID, "banded ring plan without the 16-bit slot array");
    constexpr bool kHasCol12 = std::is_same<T, float>::value && RING == (int)col12::kSlots;  // the compact form's only instantiation
    if ((c12.lo8 || c12.rec16) && (!kHasCol12 || bands != 1u || !c12.hdr || !c12.escapes))
        return fail(SMH_ERR_INVALID, "ring kernel: the compact column form is for f32 on the single-window ring of 16384 columns");
    // the plan's row ranges [lb0, lb1) (default: all of them)
    const unsigned lb0 = block_begin < n_blocks ? block_begin : n_blocks, lb1 = block_end < n_blocks ? block_end : n_blocks;
    const bool whole = lb0 == 0 && lb1 == n_blocks;
    if (!whole && dot_partials) return fail(SMH_ERR_INVALID, "ring kernel: the DOT form takes the whole plan");
    if (lb1 <= lb0) return SMH_OK;
    // entries the streaming kernel may touch: everything when the arrays are padded to a multiple of 4,
    // else only whole chunks (the rest goes to k_ring2_tail)
    const uint64_t nnz_lim = padded ? nnz : (nnz & ~uint64_t(3));
    if (resident_out) {  // (the query: nothing is enqueued)
        *resident_out = 0;
        *threads_out = Ring2Cfg<T, RING>::kThreads;
    }
    if (dot_partials && !resident_out) SMH_HIP(hipMemsetAsync(dot_partials, 0, ((size_t)n_blocks + 1) * sizeof(T), s));
    if (nnz_lim == 0) {
        if (!dot_partials && lb1 == n_blocks && !resident_out) SMH_HIP(hipMemsetAsync(y, 0, n_rows * sizeof(T), s));  // (<= 3 entries: the tail kernel below writes them)
    } else {
        const uint64_t last_chunk = (nnz_lim - 1) & ~uint64_t(3);
        dim3 grid(((lb1 - lb0) + 7u) & ~7u), block(Ring2Cfg<T, RING>::kThreads);
        constexpr size_t ring_bytes = (size_t)RING * sizeof(T);
        // dynamic LDS above 64 KiB must be allowed per kernel (idempotent, cheap)
#define SMH_R2_LAUNCH2(L, C, N, D, R)                                                                                    \
    do {                                                                                                                 \
        constexpr size_t lds_bytes = ring_bytes + (has_headers(N) ? sizeof(col12::Table) : 0);                           \
        /* once per (instantiation, DEVICE): function attributes are per device, and smh_par_* places blocks on       \
           several devices.  Bit d of the mask = device d has the opt-in; a second thread racing on the same bit only   \
           repeats an idempotent call.  (Set by the first launch, so never inside a later stream capture.) */          \
        static std::atomic<uint64_t> attr_mask{0};                                                                       \
        const uint64_t dev_bit = 1ull << (unsigned)(current_device() & 63);                                              \
        if (!(attr_mask.load(std::memory_order_acquire) & dev_bit)) {                                                    \
            SMH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_spmv_ring2<T, L, C, N, RING, D, R>),            \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));                    \
            attr_mask.fetch_or(dev_bit, std::memory_order_release);                                                      \
        }                                                                                                                \
        if (resident_out)                                                                                                \
            SMH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(resident_out, k_spmv_ring2<T, L, C, N, RING, D, R>,      \
                                                                 (int)block.x, lds_bytes));                              \
        else                                                                                                             \
            hipLaunchKernelGGL((k_spmv_ring2<T, L, C, N, RING, D, R>), grid, block, lds_bytes, s, off, col, col16, c12, val, x, y, \
                               (uint32_t)nnz_lim, last_chunk, phase_ptr, phases, bands, dot_partials, (uint32_t)lb0,     \
                               (uint32_t)(lb1 - lb0), reg_len);                                                          \
    } while (0)
#define SMH_R2_LAUNCH1(L, C, N, R)                                                               \
    do {                                                                                         \
        if (dot_partials) SMH_R2_LAUNCH2(L, C, N, true, R); else SMH_R2_LAUNCH2(L, C, N, false, R); \
    } while (0)
    /* the narrow column forms: with the table of regular phases, the kernel that reads it */
#define SMH_R2_LAUNCH0(L, C, N)                                                                 \
    do {                                                                                        \
        if (reg_len) SMH_R2_LAUNCH1(L, C, N, true); else SMH_R2_LAUNCH1(L, C, N, false);         \
    } while (0)
#define SMH_R2_LAUNCH(L, C)                                                   \
    do {                                                                      \
        if (c12.rec16) { /* (the REGK form only: see k_spmv_ring2) */         \
            if (!reg_len) return fail(SMH_ERR_INVALID, "ring kernel: the chunk records go with the table of regular phases"); \
            if constexpr (kHasCol12) SMH_R2_LAUNCH1(L, C, kRec16, true);      \
        } else if (c12.lo8) {                                                 \
            if constexpr (kHasCol12) SMH_R2_LAUNCH0(L, C, kCol12);            \
        } else if (col16) SMH_R2_LAUNCH0(L, C, kCol16);                       \
        else SMH_R2_LAUNCH1(L, C, kColU32, false);                            \
    } while (0)
        switch (lanes * 16 + chunks) {
            case 1 * 16 + 1: SMH_R2_LAUNCH(1, 1); break;
            case 1 * 16 + 2: SMH_R2_LAUNCH(1, 2); break;
            case 1 * 16 + 3: SMH_R2_LAUNCH(1, 3); break;
            case 2 * 16 + 1: SMH_R2_LAUNCH(2, 1); break;
            case 2 * 16 + 2: SMH_R2_LAUNCH(2, 2); break;
            case 4 * 16 + 1: SMH_R2_LAUNCH(4, 1); break;
            case 8 * 16 + 1: SMH_R2_LAUNCH(8, 1); break;
            case 16 * 16 + 1: SMH_R2_LAUNCH(16, 1); break;
            case 32 * 16 + 1: SMH_R2_LAUNCH(32, 1); break;
            case 64 * 16 + 1: SMH_R2_LAUNCH(64, 1); break;
            default:
                return fail(SMH_ERR_INVALID, "ring kernel: unsupported (lanes per row, chunks per lane) = (%d, %d)", lanes, chunks);
        }
#undef SMH_R2_LAUNCH
#undef SMH_R2_LAUNCH0
#undef SMH_R2_LAUNCH1
#undef SMH_R2_LAUNCH2
        SMH_HIP(hipGetLastError());
    }
    if (nnz_lim != nnz && lb1 == n_blocks && !resident_out) {  // (the last <= 3 entries belong to the last rows: with the launch that covers them)
        if (dot_partials) {
            hipLaunchKernelGGL(k_ring2_tail_dot<T>, dim3(1), dim3(64), 0, s, off, col, val, x, (const T *)y, dot_partials + n_blocks,
                               (uint64_t)n_rows, nnz_lim, (uint64_t)nnz);
            SMH_HIP(hipGetLastError());
        } else {
            SMH_TRY(launch_ring2_tail(sizeof(T) == 8 ? SMH_F64 : SMH_F32, off, col, val, x, y, n_rows, nnz_lim, nnz, s));
        }
    }
    return SMH_OK;
}

// ring_entries: what the phase plan was built for (kRingEntries; kRingEntriesWide for f32 matrices that need it).
// dot_partials != NULL (n_blocks + 1 values): the DOT form, `y` = lhs (see launch_ring2_t).
// reg_len (NULL: none; only for a plan whose phases ALL gather from the ring, use_ring == 1): one u32 per phase, the row length of
// a phase whose rows are all equally long, else 0 (k_ring_regular) -- the REGK kernel then runs, in which such a phase computes its
// row offsets instead of loading them; same chunks, same lanes, same order of FMAs.  The u32 columns have no such kernel.
// resident_out, threads_out (both or neither): the query of launch_ring2_t instead of the launch.
int launch_spmv_ring2(int dtype, int lanes, int chunks, const uint32_t *off, const uint32_t *col, const uint16_t *col16, const RingCol12 &c12,
                      const void *val, const void *x, void *y, size_t n_rows, size_t nnz, bool padded, unsigned n_blocks,
                      const uint32_t *phase_ptr, const RingPhase *phases, unsigned ring_entries, unsigned bands,
                      hipStream_t s, void *dot_partials, unsigned block_begin, unsigned block_end, const uint32_t *reg_len, int *resident_out,
                      int *threads_out) {
    if (resident_out) *resident_out = *threads_out = 0;
    if (n_rows == 0) return SMH_OK;
    if (bands != 1u && bands != 4u) return fail(SMH_ERR_INVALID, "ring kernel: %u bands", bands);
    if (dtype == SMH_F64) {
        if (ring_entries != (unsigned)kRingEntries) return fail(SMH_ERR_INVALID, "f64 ring kernel: ring of %u columns", ring_entries);
        return launch_ring2_t<double, kRingEntries>(lanes, chunks, off, col, col16, c12, (const double *)val, (const double *)x,
                                                    (double *)y, n_rows, nnz, padded, n_blocks, phase_ptr, phases, bands,
                                                    (double *)dot_partials, s, block_begin, block_end, reg_len, resident_out, threads_out);
    }
    if (ring_entries == (unsigned)kRingEntriesWide)
        return launch_ring2_t<float, kRingEntriesWide>(lanes, chunks, off, col, col16, c12, (const float *)val, (const float *)x,
                                                       (float *)y, n_rows, nnz, padded, n_blocks, phase_ptr, phases, bands,
                                                       (float *)dot_partials, s, block_begin, block_end, reg_len, resident_out, threads_out);
    if (ring_entries != (unsigned)kRingEntries) return fail(SMH_ERR_INVALID, "ring kernel: ring of %u columns", ring_entries);
    return launch_ring2_t<float, kRingEntries>(lanes, chunks, off, col, col16, c12, (const float *)val, (const float *)x, (float *)y,
                                               n_rows, nnz, padded, n_blocks, phase_ptr, phases, bands, (float *)dot_partials, s, block_begin, block_end, reg_len, resident_out, threads_out);
}

}  // namespace smh
