// spmv_many.hip -- K1m: one sweep over the matrix for KT right-hand sides (Y = A X on a device multi-vector), gfx950.
//
// The product of SparseMatrix::mvp (reference sparsematrix.rs:146-158 over sparsemat_crs.rs:102-110), once per column of X: the
// reference's mvp is generic over the vector and fixes no order ACROSS independent right-hand sides, so k products are k calls
// of it and every column is held to K1s's standard -- each product rounded, then added in storage order from T(0): bit for bit
// the reference's `sum += rhs.get(j) * val`, per column.
//
// Why: a single product on a matrix with column locality already streams the matrix at the copy ceiling; k of them read it k
// times.  K1m reads each entry ONCE per group of KT columns.  X and Y are interleaved (element i of vector c at d[i * ld + c],
// ld a multiple of 4, smh_mvec in mvec.hip), so what a thread gathers for one entry -- x[col] of KT vectors -- is one aligned
// 16-byte load (f32, KT = 4), and a row of Y leaves as one 16-byte store.
//
// The scheme is K1s's (spmv_stream.hip) widened by KT:
//   * one 256-thread workgroup per tile of 256 consecutive rows, XCD-aware tile order;
//   * the tile's entries [off[r0], off[r1]) are read as one dense run of 16-byte chunks of col and val, all chunk loads of a
//     pass issued before the first gather;
//   * per entry the KT values x[col * ld + c0 ..] are fetched with 16-byte loads and the KT ROUNDED products parked in LDS:
//     KT planes of the product stage, each with K1s's skewed index (the fold reads of a plane are K1s's: conflict-free for
//     power-of-two row lengths);
//   * after one barrier thread r folds the KT sums of row r0 + r sequentially and stores them as one row of Y (non-temporal);
//   * a tile with more entries than the stage holds is taken in passes with the KT accumulators carried (K1s's MULTI), so any
//     row length is correct and bit-exact; the arrays' unpadded tail chunk is read entry by entry.
// ceil(ld / KT) sweeps cover all columns.  Columns at and beyond k (the padding up to ld) are STORED AS +0 whatever they
// computed: a padding product 0 x Inf must not leave a NaN in storage that column operations read later.
//
// The u32 columns are streamed as they are and d_val is read directly: no derived form of the handle is involved, so
// smh_crs_update_values / scale / a values-only apply need no refresh here.  (K1s's 16-bit column codes and the value
// dictionary would save bytes per entry here too; not done.)
#include "internal.hpp"

namespace smh {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t mskew(uint32_t i) { return i + (i >> 5); }  // K1s's skew: +1 word every 32
__device__ __forceinline__ float mm_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mm_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float mm_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double mm_add(double a, double b) { return __dadd_rn(a, b); }

// KT values from a 16-byte aligned address
template <typename T, int KT> __device__ __forceinline__ void load_group(const T *p, T (&out)[KT]) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int q = 0; q < KT / 4; ++q) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(p + 4 * q);
            out[4 * q] = a.x; out[4 * q + 1] = a.y; out[4 * q + 2] = a.z; out[4 * q + 3] = a.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < KT / 2; ++q) {
            const f64x2 a = *reinterpret_cast<const f64x2 *>(p + 2 * q);
            out[2 * q] = a.x; out[2 * q + 1] = a.y;
        }
    }
}
template <typename T, int KT> __device__ __forceinline__ void store_group_nt(T *p, const T (&v)[KT]) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int q = 0; q < KT / 4; ++q) {
            f32x4 a;
            a.x = v[4 * q]; a.y = v[4 * q + 1]; a.z = v[4 * q + 2]; a.w = v[4 * q + 3];
            __builtin_nontemporal_store(a, reinterpret_cast<f32x4 *>(p + 4 * q));
        }
    } else {
#pragma unroll
        for (int q = 0; q < KT / 2; ++q) {
            f64x2 a;
            a.x = v[2 * q]; a.y = v[2 * q + 1];
            __builtin_nontemporal_store(a, reinterpret_cast<f64x2 *>(p + 2 * q));
        }
    }
}

// CAP: entries of a pass (per plane of the stage).  LDS: KT * (CAP + CAP / 32 + 8) * sizeof(T) -- see kManyCap* in
// internal.hpp: every instantiation stays at or below 66.5 KiB, so at least two workgroups share a CU's 160 KiB.
// c0: first column of this sweep's group (a multiple of KT); k: the vectors' count (columns >= k are padding).
template <typename T, int KT, int CAP>
__global__ void __launch_bounds__(kBlock)
k_spmv_many(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val, const T *__restrict__ x,
            T *__restrict__ y, uint64_t n_rows, uint64_t nnz, uint64_t nnz_readable, uint64_t n_tiles, uint64_t ld, uint32_t c0,
            uint32_t k) {
    constexpr int STRIDE = CAP + CAP / 32 + 8;  // words of one plane
    __shared__ T s_prod[KT * STRIDE];
    // bijective XCD-aware remap: XCD g (= blockIdx % 8) walks a contiguous run of tiles
    const uint64_t q = n_tiles >> 3, rm = n_tiles & 7, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const uint64_t tile = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + idx;
    const uint64_t r0 = tile * (uint64_t)kStreamRows;
    const uint64_t r1 = r0 + kStreamRows < n_rows ? r0 + kStreamRows : n_rows;
    const uint32_t tid = threadIdx.x;
    const uint64_t r = r0 + tid;
    const uint32_t o0 = off[r < r1 ? r : r1], o1 = off[r + 1 < r1 ? r + 1 : r1];
    const uint32_t k0 = off[r0], k1 = off[r1];  // tile-uniform: scalar loads
    T sum[KT];
#pragma unroll
    for (int p = 0; p < KT; ++p) sum[p] = T(0);
    const T *__restrict__ xg = x + c0;
    constexpr int NIT = (CAP + 3 + 4 * kBlock - 1) / (4 * kBlock);  // chunks per thread that cover CAP entries from an aligned start
    uint32_t ps = k0;
    do {
        const uint32_t pe = k1 - ps > (uint32_t)CAP ? ps + (uint32_t)CAP : k1;
        // everything per lane is a 32-bit position relative to the pass's aligned start `pa` (tile-uniform)
        const uint64_t pa = (uint64_t)(ps & ~3u);
        const uint32_t *__restrict__ colp = col + pa;
        const T *__restrict__ valp = val + pa;
        const uint32_t lo = ps & 3u, hi = pe - (uint32_t)pa;
        const uint64_t rd64 = nnz_readable - pa, nn64 = nnz - pa;
        const uint32_t rd = rd64 > 0x10000u ? 0x10000u : (uint32_t)rd64, nn = nn64 > 0x10000u ? 0x10000u : (uint32_t)nn64;
        uint32_t c[NIT][4] = {};
        T v[NIT][4] = {};
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const uint32_t j = 4u * tid + (uint32_t)it * (4u * kBlock);
            if (j < hi) {
                if (j + 4 <= rd) {
                    const u32x4 cc = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(colp + j));
                    c[it][0] = cc.x; c[it][1] = cc.y; c[it][2] = cc.z; c[it][3] = cc.w;
                    if constexpr (sizeof(T) == 4) {
                        const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(valp + j));
                        v[it][0] = a.x; v[it][1] = a.y; v[it][2] = a.z; v[it][3] = a.w;
                    } else {
                        const f64x2 a = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(valp + j));
                        const f64x2 b = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(valp + j + 2));
                        v[it][0] = a.x; v[it][1] = a.y; v[it][2] = b.x; v[it][3] = b.y;
                    }
                } else {  // the arrays' last, partial chunk (borrowed arrays without padding)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool in = j + e < nn;
                        c[it][e] = in ? colp[j + e] : 0u;
                        v[it][e] = in ? valp[j + e] : T(0);
                    }
                }
            }
        }
        // per chunk: the four entries' groups of x (16-byte loads), then their KT rounded products into the planes
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const uint32_t j = 4u * tid + (uint32_t)it * (4u * kBlock);
            T xv[4][KT];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t i = j + e;
#pragma unroll
                for (int p = 0; p < KT; ++p) xv[e][p] = T(0);
                if (i >= lo && i < hi) load_group<T, KT>(xg + (uint64_t)c[it][e] * ld, xv[e]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t i = j + e;
                if (i >= lo && i < hi) {
                    const uint32_t s = mskew(i - lo);
#pragma unroll
                    for (int p = 0; p < KT; ++p) s_prod[p * STRIDE + s] = mm_mul(xv[e][p], v[it][e]);
                }
            }
        }
        __syncthreads();
        // each row: storage order, one rounded add per entry and column (reference: sum += product)
        {
            uint32_t i = min(max(o0, ps), pe) - ps;
            const uint32_t iend = min(max(o1, ps), pe) - ps;
            for (; i < iend; ++i) {
                const uint32_t s = mskew(i);
#pragma unroll
                for (int p = 0; p < KT; ++p) sum[p] = mm_add(sum[p], s_prod[p * STRIDE + s]);
            }
        }
        ps = pe;
        if (ps < k1) __syncthreads();  // the next pass overwrites the stage
    } while (ps < k1);
    if (r < r1) {
#pragma unroll
        for (int p = 0; p < KT; ++p)
            if (c0 + (uint32_t)p >= k) sum[p] = T(0);  // padding columns hold +0, whatever their x held
        store_group_nt<T, KT>(y + r * ld + c0, sum);
    }
}

template <typename T>
static int launch_many_t(const uint32_t *off, const uint32_t *col, const T *val, const T *x, T *y, size_t n_rows, size_t nnz, bool padded,
                         size_t k, size_t ld, hipStream_t s) {
    const uint64_t readable = padded ? ((nnz + 3) & ~uint64_t(3)) : nnz;
    const uint64_t n_tiles = (n_rows + kStreamRows - 1) / kStreamRows;
    const dim3 grid((unsigned)n_tiles), block(kBlock);
    // A/B knob: the KT = 8 body where ld allows it (off by default: see DESIGN.md, K1m)
    static const bool kt8 = getenv("SMH_MANY_KT8") && atoi(getenv("SMH_MANY_KT8")) != 0;
    constexpr int CAP8 = sizeof(T) == 4 ? kManyCap : kManyCap / 2;
    size_t c0 = 0;
    if (kt8 && ld % 8 == 0) {
        for (; c0 < ld; c0 += 8)
            hipLaunchKernelGGL((k_spmv_many<T, 8, CAP8>), grid, block, 0, s, off, col, val, x, y, (uint64_t)n_rows, (uint64_t)nnz, readable, n_tiles,
                               (uint64_t)ld, (uint32_t)c0, (uint32_t)k);
    } else {
        for (; c0 < ld; c0 += 4)
            hipLaunchKernelGGL((k_spmv_many<T, 4, kManyCap>), grid, block, 0, s, off, col, val, x, y, (uint64_t)n_rows, (uint64_t)nnz, readable, n_tiles,
                               (uint64_t)ld, (uint32_t)c0, (uint32_t)k);
    }
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

int launch_spmv_many(int dtype, const uint32_t *off, const uint32_t *col, const void *val, const void *x, void *y, size_t n_rows, size_t nnz,
                     bool padded, size_t k, size_t ld, hipStream_t s) {
    if (n_rows == 0) return SMH_OK;
    if (dtype == SMH_F64) return launch_many_t<double>(off, col, (const double *)val, (const double *)x, (double *)y, n_rows, nnz, padded, k, ld, s);
    return launch_many_t<float>(off, col, (const float *)val, (const float *)x, (float *)y, n_rows, nnz, padded, k, ld, s);
}

}  // namespace smh
