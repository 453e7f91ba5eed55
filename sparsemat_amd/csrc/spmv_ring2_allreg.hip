// spmv_ring2_allreg.hip -- K1r's all-regular form (k_spmv_ring2_allreg, spmv_ring2_kernel.hpp): its instantiations and their launch.
// A source of its own so that they compile beside spmv_ring2.hip, the build's longest compile, and not after it.
//
// f32 on the 16384-slot ring, no DOT, the three narrow column forms, the (lanes, chunks) pairs of launch_ring2_t's switch; workgroups
// of kRingAllregThreads = 768 threads, __launch_bounds__(768, 6): two workgroups per CU are 24 wavefronts, 6 per SIMD, which needs
// <= 80 VGPRs.  By the compiler's resource remarks every pair meets that without scratch in all three
// column forms (37-74 VGPRs) except (2, 2), which spills 4-10 VGPRs in each of them: it has no instantiation here, ring2_allreg_has()
// says so and the dispatch keeps the REGK kernel for it.
#include "spmv_ring2_kernel.hpp"

#include <atomic>

namespace smh {

bool ring2_allreg_has(int lanes, int chunks) {
    switch (lanes * 16 + chunks) {
        case 1 * 16 + 1: case 1 * 16 + 2: case 1 * 16 + 3: case 2 * 16 + 1:
        case 4 * 16 + 1: case 8 * 16 + 1: case 16 * 16 + 1: case 32 * 16 + 1: case 64 * 16 + 1: return true;
        default: return false;
    }
}

int launch_spmv_ring2_allreg(int lanes, int chunks, const uint32_t *off, const uint32_t *col, const uint16_t *col16, const RingCol12 &c12,
                             const float *val, const float *x, float *y, size_t n_rows, size_t nnz, bool padded, unsigned n_blocks,
                             const uint32_t *phase_ptr, const RingPhase *phases, hipStream_t s, unsigned block_begin, unsigned block_end,
                             const uint32_t *reg_len, int *resident_out, int *threads_out) {
    constexpr int RING = kRingEntries, THREADS = kRingAllregThreads;
    if (resident_out) {  // (the query: nothing is enqueued)
        *resident_out = 0;
        *threads_out = THREADS;
    }
    if (n_rows == 0) return SMH_OK;
    if (!reg_len) return fail(SMH_ERR_INVALID, "ring kernel: the all-regular form goes with the table of regular phases");
    if ((c12.lo8 || c12.rec16) ? (!c12.hdr || !c12.escapes) : !col16)
        return fail(SMH_ERR_INVALID, "ring kernel: the all-regular form streams the chunk records, the compact column form or the 16-bit columns");
    // the plan's row ranges [lb0, lb1), the entries the kernel may touch and the tail: as launch_ring2_t has them
    const unsigned lb0 = block_begin < n_blocks ? block_begin : n_blocks, lb1 = block_end < n_blocks ? block_end : n_blocks;
    if (lb1 <= lb0) return SMH_OK;
    const uint64_t nnz_lim = padded ? nnz : (nnz & ~uint64_t(3));
    if (nnz_lim == 0) {
        if (lb1 == n_blocks && !resident_out) SMH_HIP(hipMemsetAsync(y, 0, n_rows * sizeof(float), s));
    } else {
        const uint64_t last_chunk = (nnz_lim - 1) & ~uint64_t(3);
        dim3 grid(((lb1 - lb0) + 7u) & ~7u), block(THREADS);
#define SMH_R2A_LAUNCH1(L, C, N)                                                                                          \
    do {                                                                                                                  \
        constexpr size_t lds_bytes = (size_t)RING * sizeof(float) + (has_headers(N) ? sizeof(col12::Table) : 0);          \
        /* the opt-in to dynamic LDS above 64 KiB, once per (instantiation, device): see launch_ring2_t */              \
        static std::atomic<uint64_t> attr_mask{0};                                                                        \
        const uint64_t dev_bit = 1ull << (unsigned)(current_device() & 63);                                               \
        if (!(attr_mask.load(std::memory_order_acquire) & dev_bit)) {                                                     \
            SMH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_spmv_ring2_allreg<float, L, C, N, RING, THREADS>), \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));                     \
            attr_mask.fetch_or(dev_bit, std::memory_order_release);                                                       \
        }                                                                                                                 \
        if (resident_out)                                                                                                 \
            SMH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(resident_out, k_spmv_ring2_allreg<float, L, C, N, RING, THREADS>, \
                                                                 THREADS, lds_bytes));                                    \
        else                                                                                                              \
            hipLaunchKernelGGL((k_spmv_ring2_allreg<float, L, C, N, RING, THREADS>), grid, block, lds_bytes, s, off, col16, c12, val, x, y, \
                               (uint32_t)nnz_lim, last_chunk, phase_ptr, phases, (uint32_t)lb0, (uint32_t)(lb1 - lb0), reg_len); \
    } while (0)
#define SMH_R2A_LAUNCH(L, C)                                  \
    do {                                                      \
        if (c12.rec16) SMH_R2A_LAUNCH1(L, C, kRec16);         \
        else if (c12.lo8) SMH_R2A_LAUNCH1(L, C, kCol12);      \
        else SMH_R2A_LAUNCH1(L, C, kCol16);                   \
    } while (0)
        switch (lanes * 16 + chunks) {  // (the pairs of ring2_allreg_has)
            case 1 * 16 + 1: SMH_R2A_LAUNCH(1, 1); break;
            case 1 * 16 + 2: SMH_R2A_LAUNCH(1, 2); break;
            case 1 * 16 + 3: SMH_R2A_LAUNCH(1, 3); break;
            case 2 * 16 + 1: SMH_R2A_LAUNCH(2, 1); break;
            case 4 * 16 + 1: SMH_R2A_LAUNCH(4, 1); break;
            case 8 * 16 + 1: SMH_R2A_LAUNCH(8, 1); break;
            case 16 * 16 + 1: SMH_R2A_LAUNCH(16, 1); break;
            case 32 * 16 + 1: SMH_R2A_LAUNCH(32, 1); break;
            case 64 * 16 + 1: SMH_R2A_LAUNCH(64, 1); break;
            default:
                return fail(SMH_ERR_INVALID, "ring kernel: the all-regular form has no (lanes per row, chunks per lane) = (%d, %d)", lanes, chunks);
        }
#undef SMH_R2A_LAUNCH
#undef SMH_R2A_LAUNCH1
        SMH_HIP(hipGetLastError());
    }
    if (nnz_lim != nnz && lb1 == n_blocks && !resident_out)
        SMH_TRY(launch_ring2_tail(SMH_F32, off, col, val, x, y, n_rows, nnz_lim, nnz, s));
    return SMH_OK;
}

}  // namespace smh
