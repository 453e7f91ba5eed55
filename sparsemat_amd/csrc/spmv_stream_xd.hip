// spmv_stream_xd.hip -- K1s "XD": the CSR-stream kernel for stencil-like matrices with everything a thread would have to compute
// per entry moved into the build.  Same product, same arithmetic and same ORDER as K1s (spmv_stream.hip; reference
// sparsematrix.rs:146-158 over sparsemat_crs.rs:102-110): products rounded, then added to the row's sum in storage order, one
// rounded add per entry, starting from +0 -- bit-exact against the reference loop.
//
// Why: K1s with x staged in LDS (XS) is bound by vector-ALU issue, not by bytes -- a wavefront instruction occupies its 16-lane
// SIMD for 4 cycles, a 256-row tile costs each of its four wavefronts ~400 of them, 2048 tiles per CU: 1.37 ms of issue time on
// the 512^3 Laplacian for 1.30 ms measured.  Per entry the XS body spent 6 instructions turning a 16-bit column code (interval,
// offset) into an LDS address, 7 on where the product goes (position relative to the tile, range test, bank skew, select), and
// the row sums walked a skewed stage in two loops with a dependent LDS round trip per step.  Here
//   * the code array holds the BYTE OFFSET of x[col] inside the tile's LDS stage of x (the stage's layout is a function of
//     the tile's interval table alone, so the build can know it): decode = extracting 16 bits;
//   * a thread's four products of a chunk leave as ONE 16-byte LDS store at the chunk's own position (the stage is not skewed
//     and covers both chunks of every thread, so slots before the tile's first / after its last entry need no test: they receive
//     products nobody reads);
//   * the chunk loads are buffer loads whose descriptors end with the tile's entries: no branches, no tail path;
//   * a row's first 8 products are read with 8 independent LDS loads and added under a lane mask (rows beyond 8 entries continue in
//     a loop); the row-length prefix sum is a DPP scan.
// Without the skew the row sums of rows of EVEN length collide in LDS (stride 8 -> 8 lanes per bank); the handle takes this form
// only when most rows have an odd length -- every stencil with a diagonal: 5, 7, 9, 27 points -- (crs_forms.hip, stream_cfg).
#include <atomic>

#include "internal.hpp"
#include "stream_stage.hpp"

namespace smh {

namespace {

typedef uint32_t xd_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t xd_u2 __attribute__((ext_vector_type(2)));
typedef float xd_f4 __attribute__((ext_vector_type(4)));
typedef double xd_d2 __attribute__((ext_vector_type(2)));
constexpr int kXdRsrc = 0x00020000;  // dword 3 of a raw buffer descriptor on gfx9 (32-bit data format)

template <int CTRL, int ROWS> __device__ __forceinline__ uint32_t xd_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xF, false);  // lanes without a source receive 0
}
// inclusive prefix sum over the wavefront
__device__ __forceinline__ uint32_t xd_wave_scan(uint32_t v) {
    v += xd_dpp<0x111, 0xF>(v);  // row_shr:1
    v += xd_dpp<0x112, 0xF>(v);  // row_shr:2
    v += xd_dpp<0x114, 0xF>(v);  // row_shr:4
    v += xd_dpp<0x118, 0xF>(v);  // row_shr:8
    v += xd_dpp<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
    v += xd_dpp<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3
    // (opaque from here on.  Seen as its argument + six DPP terms, `incl - my_len` of the row sums is rewritten as the sum of those
    // terms; they then live across blocks and the six moves are no longer folded into their adds: 13 instructions, 6 registers)
    asm("" : "+v"(v));
    return v;
}

constexpr int kXdSlots = 2 * 4 * kBlock;  // product slots of a tile: two 4-entry chunks per thread (kStreamCapSmall + 3 <= 2048)
static_assert(kStreamCapSmall + 3 <= kXdSlots, "a tile's entries from an aligned start fit two chunks per thread");

// K1s XD-V: the VALUE DICTIONARY form.  A stage offset is a multiple of sizeof(T) below the stage's size, so a 16-bit code has bits
// to spare -- the low log2(sizeof T) ones and those above the stage: 5 bits with the 2048-entry stage (f32 and f64), 4 with the
// 4096-entry one.  When the matrix holds no more than 32 / 16 DISTINCT values (bit patterns) -- every constant-coefficient stencil,
// every unweighted graph Laplacian or adjacency matrix; BASELINE C4 has two, 6 and -1 -- those bits name the entry's value in a
// dictionary the kernel keeps in LDS, and the value array is not read at all: 2 bytes per entry leave HBM instead of 6 (f32) / 10
// (f64).  The product is x times the very same bit pattern as before, the adds are in storage order: still bit for bit the
// reference's result.  (stream_cfg in crs_forms.hip decides; k_value_dict_* below build the dictionary, exactly, or say that it does not exist.)
// (the code's bits: stream_stage.hpp.  Dictionaries small enough for the bits ABOVE the offset -- every stencil's -- keep the index
// there alone: one shift instead of three operations, VD == 2 below.)

// ---- one tile, step by step ---------------------------------------------------------------------------------------------------------
// What a thread holds of a tile between requesting it and summing its row.  The per-tile kernel has one set and takes the steps once;
// the persistent kernel has two and requests the next tile's while it multiplies the current one's.
// XS: 16-byte chunks of x per thread the tile's stage holds (2 or 4); VALS: the value array is read (no dictionary)
template <typename T, int XS, bool VALS>
struct XdTileRegs {
    uint32_t k0, pa, my_len, xs_tot;
    uint64_t r0, tile;
    T dl;
    T xr[XS][4];
    uint32_t xpiece[XS][2];  // f64: the two 16-byte pieces (2 entries each) of the stage this thread fills
    xd_u2 cw[2];
    T v[VALS ? 2 : 1][4];
    uint32_t epos[2][2];  // f64: the entry positions (relative to pa) of the thread's two 2-entry pieces
};

// step 1: everything of `tile` a thread needs, requested -- table words, row length, dot lhs, the x chunks, then the tile's entries
template <typename T, bool DOT, int XS, bool VALS>
__device__ __forceinline__ void xd_request(XdTileRegs<T, XS, VALS> &R, uint64_t tile, const T *__restrict__ val, const T *__restrict__ x,
                                           uint64_t n_rows, const uint16_t *__restrict__ scode, const uint32_t *__restrict__ cwin,
                                           const uint8_t *__restrict__ len8, const uint32_t *__restrict__ tbase, const T *__restrict__ dot_lhs) {
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t wbase = tid & ~(uint32_t)(kWave - 1);  // first thread of this wavefront
    R.tile = tile;
    R.r0 = tile * (uint64_t)kStreamRows;
    const uint32_t k0 = tbase[tile], k1 = tbase[tile + 1];  // tile-uniform: scalar loads
    R.k0 = k0;
    R.my_len = len8[R.r0 + tid];  // (the byte array is padded to whole tiles with zeros)
    R.dl = T(0);
    if constexpr (DOT) R.dl = R.r0 + tid < n_rows ? dot_lhs[R.r0 + tid] : T(0);  // requested now: its latency hides behind the tile
    // ---- the tile's intervals of x: 16-byte chunks, requested before the tile's own entries (they are needed first) ----
    const stage::Layout lay = stage::layout(cwin + 8 * tile);  // scalar loads
    R.xs_tot = lay.chunks();  // (<= XS * kBlock chunks, inside x: checked by the host)
    // f64: a thread's 32 bytes (of x, of the values, of the products) are TWO 16-byte pieces, and a wavefront's lanes take piece
    // l and piece 64 + l of its 128 -- each load / store instruction then covers 1 KiB of contiguous bytes.  With 32 contiguous
    // bytes per lane (rounds 2-3) each of the two instructions touched every line and used half of it: what kept K1r's f64 kernel
    // at 0.8 of its f32 rate did the same here.  Which thread moves which piece changes no arithmetic: the
    // products land in the same stage slots and are added in storage order as before (bit-exact).
#pragma unroll
    for (int u = 0; u < XS; ++u) {
        R.xr[u][0] = R.xr[u][1] = R.xr[u][2] = R.xr[u][3] = T(0);
        if constexpr (sizeof(T) == 4) {
            const uint32_t j = tid + (uint32_t)u * kBlock;
            if (j < R.xs_tot) {
                const xd_f4 a = *reinterpret_cast<const xd_f4 *>(x + 4ull * (uint64_t)lay.x_chunk(j));
                R.xr[u][0] = a.x; R.xr[u][1] = a.y; R.xr[u][2] = a.z; R.xr[u][3] = a.w;
            }
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t pi = 2u * ((uint32_t)u * kBlock + wbase) + (uint32_t)h * kWave + lane;  // piece of the stage
                const uint32_t j = pi >> 1;                                                            // its chunk
                R.xpiece[u][h] = pi;
                if (j < R.xs_tot) {
                    const xd_d2 a = *reinterpret_cast<const xd_d2 *>(x + 4ull * (uint64_t)lay.x_chunk(j) + 2u * (pi & 1u));
                    R.xr[u][2 * h] = a.x; R.xr[u][2 * h + 1] = a.y;
                }
            }
        }
    }
    // ---- the tile's entries: two chunks per thread from the aligned start `pa`; a descriptor that ends with the tile's last
    // entry makes every slot beyond it read as zero (code 0: the stage's first entry; value 0) ----
    const uint32_t pa = k0 & ~3u, hi = k1 - pa;  // hi <= kXdSlots (kStreamCapSmall, checked by the host)
    R.pa = pa;
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void *)(scode + pa), 0, (int)(((hi + 3u) & ~3u) * 2u), kXdRsrc);
    __amdgpu_buffer_rsrc_t rv = rc;  // (not used without the values)
    if constexpr (VALS) rv = __builtin_amdgcn_make_buffer_rsrc((void *)(val + pa), 0, (int)(hi * (uint32_t)sizeof(T)), kXdRsrc);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if constexpr (VALS) R.v[it][0] = R.v[it][1] = R.v[it][2] = R.v[it][3] = T(0);
        if constexpr (sizeof(T) == 4) {
            const uint32_t j = 4u * tid + (uint32_t)it * (4u * kBlock);
            R.cw[it] = __builtin_bit_cast(xd_u2, __builtin_amdgcn_raw_buffer_load_b64(rc, (int)(j * 2u), 0, 2 /* nt */));
            if constexpr (VALS) {
                const xd_f4 a = __builtin_bit_cast(xd_f4, __builtin_amdgcn_raw_buffer_load_b128(rv, (int)(j * 4u), 0, 2));
                R.v[it][0] = a.x; R.v[it][1] = a.y; R.v[it][2] = a.z; R.v[it][3] = a.w;
            }
        } else {
            const uint32_t e0p = 4u * ((uint32_t)it * kBlock + wbase) + 2u * lane, e1p = e0p + 2u * kWave;
            R.epos[it][0] = e0p; R.epos[it][1] = e1p;
            R.cw[it].x = __builtin_amdgcn_raw_buffer_load_b32(rc, (int)(e0p * 2u), 0, 2 /* nt */);
            R.cw[it].y = __builtin_amdgcn_raw_buffer_load_b32(rc, (int)(e1p * 2u), 0, 2);
            if constexpr (VALS) {
                const xd_d2 a = __builtin_bit_cast(xd_d2, __builtin_amdgcn_raw_buffer_load_b128(rv, (int)(e0p * 8u), 0, 2));
                const xd_d2 b = __builtin_bit_cast(xd_d2, __builtin_amdgcn_raw_buffer_load_b128(rv, (int)(e1p * 8u), 0, 2));
                R.v[it][0] = a.x; R.v[it][1] = a.y; R.v[it][2] = b.x; R.v[it][3] = b.y;
            }
        }
    }
}

// step 2: x into its stage
template <typename T, int XS, bool VALS>
__device__ __forceinline__ void xd_fill_stage(const XdTileRegs<T, XS, VALS> &R, T *s_xs) {
#pragma unroll
    for (int u = 0; u < XS; ++u) {
        if constexpr (sizeof(T) == 4) {
            const uint32_t j = threadIdx.x + (uint32_t)u * kBlock;
            if (j < R.xs_tot) {
                xd_f4 a; a.x = R.xr[u][0]; a.y = R.xr[u][1]; a.z = R.xr[u][2]; a.w = R.xr[u][3];
                *reinterpret_cast<xd_f4 *>(&s_xs[4u * j]) = a;
            }
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if ((R.xpiece[u][h] >> 1) < R.xs_tot) {
                    xd_d2 a; a.x = R.xr[u][2 * h]; a.y = R.xr[u][2 * h + 1];
                    *reinterpret_cast<xd_d2 *>(&s_xs[2u * R.xpiece[u][h]]) = a;
                }
        }
    }
}

// step 3: products -- x from the stage by byte offset, four products per 16-byte store at the chunk's own position.
// VD: the codes carry value-dictionary indices -- 1: in the low and the high spare bits, 2: in the high ones alone
template <typename T, int XS, int VD, bool VALS>
__device__ __forceinline__ void xd_products(const XdTileRegs<T, XS, VALS> &R, const T *s_xs, const T *s_dict, T *s_prod) {
    static_assert(VALS == (VD == 0), "an entry's value comes from the value array or from the dictionary");
    const char *xs_bytes = reinterpret_cast<const char *>(s_xs);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        T p[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t cword = (e >> 1) ? R.cw[it].y : R.cw[it].x;
            const uint32_t code = (e & 1) ? (cword >> 16) : (cword & 0xFFFFu);
            if constexpr (VD) {
                // (a slot past the tile reads code 0: stage entry 0 times dictionary entry 0 -- never added to any row)
                const uint32_t vi = VD == 2 ? stage::code_value_high(code, sizeof(T), XS) : stage::code_value(code, sizeof(T), XS);
                p[e] = stage::mul(*reinterpret_cast<const T *>(xs_bytes + stage::code_ofs(code, sizeof(T), XS)), s_dict[vi]);
            } else {
                p[e] = stage::mul(*reinterpret_cast<const T *>(xs_bytes + code), R.v[it][e]);
            }
        }
        if constexpr (sizeof(T) == 4) {
            const uint32_t j = 4u * threadIdx.x + (uint32_t)it * (4u * kBlock);
            xd_f4 a; a.x = p[0]; a.y = p[1]; a.z = p[2]; a.w = p[3];
            *reinterpret_cast<xd_f4 *>(&s_prod[j]) = a;
        } else {
            xd_d2 a, b; a.x = p[0]; a.y = p[1]; b.x = p[2]; b.y = p[3];
            *reinterpret_cast<xd_d2 *>(&s_prod[R.epos[it][0]]) = a;
            *reinterpret_cast<xd_d2 *>(&s_prod[R.epos[it][1]]) = b;
        }
    }
}

// step 4: the row's sum in storage order, one rounded add per entry (reference: sum += product), and its store.  incl: the wavefront's
// inclusive scan of the row lengths, s_wtot: the wavefronts' totals.  Returns (DOT) the wavefront's share of lhs . (A x) in lane 63 --
// fixed order: lanes by the DPP scan network, as K1s; the caller adds the wavefronts in index order
template <typename T, bool DOT, int XS, bool VALS>
__device__ __forceinline__ T xd_row_sum(const XdTileRegs<T, XS, VALS> &R, uint32_t incl, uint32_t wave, const uint32_t *s_wtot, const T *s_prod,
                                       T *__restrict__ y, uint64_t n_rows) {
    uint32_t before = 0;  // entries of the tile in the waves before this one (wave-uniform)
#pragma unroll
    for (int ww = 0; ww < kBlock / kWave - 1; ++ww) before += (uint32_t)ww < wave ? s_wtot[ww] : 0u;
    const T *pp = s_prod + ((R.k0 - R.pa) + before + (incl - R.my_len));
    T q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = pp[i];
    T acc = T(0);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if ((uint32_t)i < R.my_len) acc = stage::add(acc, q[i]);
    for (uint32_t i = 8; i < R.my_len; ++i) acc = stage::add(acc, pp[i]);
    const uint64_t r = R.r0 + threadIdx.x;
    if (r < n_rows && (!DOT || y)) __builtin_nontemporal_store(acc, &y[r]);  // (DOT with y == NULL: only lhs . (A x) is wanted)
    T d = T(0);
    if constexpr (DOT) {
        if (r < n_rows && (y || R.my_len)) d += R.dl * acc;  // (as K1s: 0 + the product; inner_prod, y == NULL: not of a row without entries)
        d = wave_sum_to_lane63(d);
    }
    return d;
}

// the wavefronts' shares of a tile's dot, added in index order by thread 0
template <typename T>
__device__ __forceinline__ void xd_fold_dot(const T *s_red, T *__restrict__ dot_partials, uint64_t tile) {
    if (threadIdx.x == 0) {
        T t = T(0);
#pragma unroll
        for (int ww = 0; ww < kBlock / kWave; ++ww) t += s_red[ww];
        dot_partials[tile] = t;
    }
}

// ---- K1s XD, one workgroup per tile: the four steps once.  VD = 0 reads the value array ---------------------------------------------
template <typename T, bool DOT, int XS, int VD = 0>
__global__ void __launch_bounds__(kBlock)
k_spmv_stream_xd(const T *__restrict__ val, const T *__restrict__ x, T *__restrict__ y, uint64_t n_rows, uint64_t n_tiles,
                 T *__restrict__ dot_partials, const uint16_t *__restrict__ scode, const uint32_t *__restrict__ cwin,
                 const uint8_t *__restrict__ len8, const uint32_t *__restrict__ tbase, const T *__restrict__ dot_lhs, uint64_t tile0,
                 const T *__restrict__ dict = nullptr) {
    constexpr int kXsCap = XS * kBlock * 4;  // entries of x the stage holds (2048 / 4096)
    __shared__ T s_dict[VD ? 32 : 1];
    // (the dictionary array has 32 entries whatever its fill.  Requested by EVERY thread, without a branch, and put into the LDS only with
    // the stage of x below: inside `if (tid < 32)` the compiler waits for the load on the spot -- a whole memory round trip for the first
    // wavefront before it has requested anything else, and the workgroup's barrier waits for that wavefront.)
    T dict_v = T(0);
    if constexpr (VD) dict_v = dict[threadIdx.x & 31u];
    __shared__ __attribute__((aligned(16))) T s_xs[kXsCap];
    __shared__ __attribute__((aligned(16))) T s_prod[kXdSlots + 8];  // (+8: a row's eight unconditional reads may pass the tile's end)
    __shared__ uint32_t s_wtot[kBlock / kWave];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid / kWave));
    const uint64_t tile = tile0 + stage::xcd_run(n_tiles, blockIdx.x & 7).first + (blockIdx.x >> 3);
    XdTileRegs<T, XS, VD == 0> R;
    xd_request<T, DOT>(R, tile, val, x, n_rows, scode, cwin, len8, tbase, dot_lhs);
    // row boundaries: prefix sum of the byte lengths (its cross-wave part rides on the barrier below)
    const uint32_t incl = xd_wave_scan(R.my_len);
    if (lane == kWave - 1) s_wtot[wave] = incl;
    xd_fill_stage(R, s_xs);
    if constexpr (VD) {
        if (tid < 32u) s_dict[tid] = dict_v;
    }
    __syncthreads();
    xd_products<T, XS, VD>(R, s_xs, s_dict, s_prod);
    __syncthreads();
    const T d = xd_row_sum<T, DOT>(R, incl, wave, s_wtot, s_prod, y, n_rows);
    if constexpr (DOT) {
        __shared__ T s_red[kBlock / kWave];
        if (lane == kWave - 1) s_red[wave] = d;
        __syncthreads();
        xd_fold_dot(s_red, dot_partials, tile);
    }
}

// ---- K1s XD-V on PERSISTENT workgroups ------------------------------------------------------------------------------------------
// With the value array gone the kernel above is bound by LATENCY: a workgroup lives 2.85 us -- the two dependent memory round trips of
// its tile (tile table -> codes and x chunks) -- at full occupancy (profiles/r04_k1s_value_dictionary.log).  Here a workgroup walks a
// contiguous run of tiles and the NEXT tile's table entries, codes, x chunks and row lengths are on their way while the current tile is
// multiplied and summed: the same four steps per tile (bit-exact), two barriers per tile as before; two register sets alternate.
// Its own: the run a workgroup takes, s_wtot / s_red by tile parity, and the dot's fold deferred past the next barrier.
template <typename T, bool DOT, int XS, int VD>
__global__ void __launch_bounds__(kBlock)
k_spmv_stream_xdp(const T *__restrict__ x, T *__restrict__ y, uint64_t n_rows, uint64_t n_tiles, T *__restrict__ dot_partials,
                  const uint16_t *__restrict__ scode, const uint32_t *__restrict__ cwin, const uint8_t *__restrict__ len8,
                  const uint32_t *__restrict__ tbase, const T *__restrict__ dot_lhs, uint64_t tile0, const T *__restrict__ dict) {
    static_assert(VD == 1 || VD == 2, "the persistent form exists for the value-dictionary kernels");
    constexpr int kXsCap = XS * kBlock * 4;
    __shared__ T s_dict[32];
    __shared__ __attribute__((aligned(16))) T s_xs[kXsCap];
    __shared__ __attribute__((aligned(16))) T s_prod[kXdSlots + 8];
    __shared__ uint32_t s_wtot[2][kBlock / kWave];  // (by tile parity: a fast wavefront stages the next tile while a slow one still sums)
    __shared__ T s_red[2][kBlock / kWave];          // (by tile parity too: folded one barrier later, see below)
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid / kWave));
    if (tid < 32u) s_dict[tid] = dict[tid];
    // XCD g (= blockIdx % 8) owns a contiguous eighth of the launch's tiles, its workgroups contiguous runs of those
    const stage::XcdRun mine = stage::xcd_run(n_tiles, blockIdx.x & 7);
    const uint64_t wgx = gridDim.x >> 3, j_wg = blockIdx.x >> 3;
    const uint64_t per = (mine.count + wgx - 1) / wgx;
    const uint64_t t_begin = mine.first + j_wg * per;
    const uint64_t t_end = t_begin + per < mine.first + mine.count ? t_begin + per : mine.first + mine.count;
    if (t_begin >= t_end) return;  // (whole workgroup, before any barrier)
    typedef XdTileRegs<T, XS, false> Regs;
    auto request = [&](Regs &R, uint64_t t) {  // t: index inside the launch
        xd_request<T, DOT>(R, tile0 + t, (const T *)nullptr, x, n_rows, scode, cwin, len8, tbase, dot_lhs);
    };
    // one tile with its registers R, prefetching tile t_next into N between the two barriers.  The wavefronts' shares of the PREVIOUS
    // tile's dot are folded by thread 0 AFTER the first barrier here, which the workgroup passes anyway (a closing one after the last
    // tile): a barrier of its own per tile, with one thread folding behind it while 255 wait at the next, cost the f32 solver 0.25 ms
    // per iteration
    auto tile_body = [&](Regs &R, Regs &N, uint64_t t_next, uint32_t par, bool first) {
        const uint32_t incl = xd_wave_scan(R.my_len);
        if (lane == kWave - 1) s_wtot[par][wave] = incl;
        xd_fill_stage(R, s_xs);
        __syncthreads();
        if constexpr (DOT) {
            if (!first) xd_fold_dot(s_red[par ^ 1u], dot_partials, R.tile - 1);  // (a workgroup's tiles are consecutive)
        }
        request(N, t_next);  // (always: no branch around the loads; the last tile is simply requested once more)
        xd_products<T, XS, VD>(R, s_xs, s_dict, s_prod);
        __syncthreads();
        const T d = xd_row_sum<T, DOT>(R, incl, wave, s_wtot[par], s_prod, y, n_rows);
        if constexpr (DOT) {
            if (lane == kWave - 1) s_red[par][wave] = d;
        }
    };
    Regs A, B;
    const uint64_t t_last = t_end - 1;
    request(A, t_begin);
    uint32_t last_par = 0;
    for (uint64_t t = t_begin;;) {
        tile_body(A, B, t + 1 < t_end ? t + 1 : t_last, 0u, t == t_begin);
        last_par = 0;
        if (++t >= t_end) break;
        tile_body(B, A, t + 1 < t_end ? t + 1 : t_last, 1u, false);
        last_par = 1;
        if (++t >= t_end) break;
    }
    if constexpr (DOT) {
        __syncthreads();
        xd_fold_dot(s_red[last_par], dot_partials, tile0 + t_last);
    }
}

// stage offsets: code = BYTES from the start of the tile's LDS stage of x to x[column]
__global__ void __launch_bounds__(kBlock)
k_stream_stage_codes(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const uint32_t *__restrict__ win,
                     uint64_t n_rows, uint64_t n_tiles, uint32_t elem_bytes, uint16_t *__restrict__ code) {
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const stage::Layout lay = stage::layout(win + 8 * t);
        const uint64_t r0 = t * kStreamRows, r1 = r0 + kStreamRows < n_rows ? r0 + kStreamRows : n_rows;
        const uint64_t k0 = off[r0], k1 = off[r1];
        for (uint64_t k = k0 + threadIdx.x; k < k1; k += kBlock) code[k] = (uint16_t)(lay.entry(col[k]) * elem_bytes);
    }
}

// ---- the value dictionary (see K1s XD-V above) --------------------------------------------------------------------------------------
// Distinct BIT PATTERNS of val[0..nnz), at most kXdDictCap of them, exactly -- or the verdict that there are more.  Phase 1: every
// workgroup collects the patterns of its share in an LDS table (compare-and-swap into the first empty slot) and leaves the table in
// global memory; a workgroup whose table overflows raises a flag that makes everybody stop (a matrix with arbitrary values is found
// out within the first few hundred entries of every workgroup).  Phase 2: one workgroup merges the tables the same way, sorts the
// result by bit pattern (the dictionary must not depend on who came first) and publishes it.
constexpr uint32_t kXdDictCap = 32;
// (a slot is empty while it holds this pattern -- a NaN payload no computation produces; a matrix that does hold it is reported as
// "more than the dictionary holds", which costs it nothing but this optimisation)
template <typename T> struct XdPat;
template <> struct XdPat<float> { typedef uint32_t U; static constexpr U kEmpty = 0x7FC5A5A5u; };
template <> struct XdPat<double> { typedef unsigned long long U; static constexpr U kEmpty = 0x7FF8A5A55A5AA5A5ull; };

template <typename U>
__device__ __forceinline__ bool xd_dict_insert(U *tab, U pat, U empty) {  // false: the table is full and does not hold pat
    for (uint32_t i = 0; i < kXdDictCap; ++i) {
        const U seen = tab[i];
        if (seen == pat) return true;
        if (seen == empty) {
            const U old = atomicCAS(tab + i, empty, pat);
            if (old == empty || old == pat) return true;
        }
    }
    return false;
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_value_dict_collect(const T *__restrict__ val, uint64_t nnz, typename XdPat<T>::U *__restrict__ wg_tables, uint32_t *__restrict__ overflow) {
    typedef typename XdPat<T>::U U;
    __shared__ U tab[kXdDictCap];
    if (threadIdx.x < kXdDictCap) tab[threadIdx.x] = XdPat<T>::kEmpty;
    __syncthreads();
    const U *bits = reinterpret_cast<const U *>(val);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nnz; i += (uint64_t)gridDim.x * kBlock) {
        if (*(volatile uint32_t *)overflow) break;  // somebody found a 33rd value: nothing left to learn
        const U pat = bits[i];
        if (pat == XdPat<T>::kEmpty || !xd_dict_insert<U>(tab, pat, XdPat<T>::kEmpty)) { atomicOr(overflow, 1u); break; }
    }
    __syncthreads();
    if (threadIdx.x < kXdDictCap) wg_tables[(uint64_t)blockIdx.x * kXdDictCap + threadIdx.x] = tab[threadIdx.x];
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_value_dict_merge(const typename XdPat<T>::U *__restrict__ wg_tables, uint32_t n_tables, T *__restrict__ dict, uint32_t *__restrict__ count,
                   uint32_t *__restrict__ overflow) {
    typedef typename XdPat<T>::U U;
    __shared__ U tab[kXdDictCap];
    __shared__ uint32_t s_over;
    if (threadIdx.x < kXdDictCap) tab[threadIdx.x] = XdPat<T>::kEmpty;
    if (threadIdx.x == 0) s_over = *overflow;
    __syncthreads();
    if (!s_over) {
        for (uint32_t i = threadIdx.x; i < n_tables * kXdDictCap; i += kBlock) {
            const U pat = wg_tables[i];
            if (pat != XdPat<T>::kEmpty && !xd_dict_insert<U>(tab, pat, XdPat<T>::kEmpty)) s_over = 1u;  // (benign race: any writer writes 1)
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t n = 0;
        U sorted[kXdDictCap];
        for (uint32_t i = 0; i < kXdDictCap; ++i)
            if (tab[i] != XdPat<T>::kEmpty) sorted[n++] = tab[i];
        for (uint32_t i = 1; i < n; ++i) {  // insertion sort by bit pattern: <= 32 entries, once per matrix
            const U v = sorted[i];
            uint32_t j = i;
            while (j > 0 && sorted[j - 1] > v) { sorted[j] = sorted[j - 1]; --j; }
            sorted[j] = v;
        }
        U *out = reinterpret_cast<U *>(dict);
        for (uint32_t i = 0; i < kXdDictCap; ++i) out[i] = i < n ? sorted[i] : (U)0;
        *count = s_over ? 0u : n;
        *overflow = s_over;
    }
}

// code[k] |= the dictionary index of val[k], spread over the code's spare bits (low `low` bits, then the bits from `high_shift` up)
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_value_dict_encode(const T *__restrict__ val, uint64_t nnz, const T *__restrict__ dict, uint32_t n, uint32_t low, uint32_t high_shift,
                    uint16_t *__restrict__ code) {
    typedef typename XdPat<T>::U U;
    __shared__ U tab[kXdDictCap];
    if (threadIdx.x < kXdDictCap) tab[threadIdx.x] = reinterpret_cast<const U *>(dict)[threadIdx.x];
    __syncthreads();
    const U *bits = reinterpret_cast<const U *>(val);
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < nnz; k += (uint64_t)gridDim.x * kBlock) {
        const U pat = bits[k];
        uint32_t idx = 0;
        for (uint32_t i = 0; i < n; ++i) idx = tab[i] == pat ? i : idx;  // (every pattern is in the dictionary: it was built from these values)
        code[k] = (uint16_t)stage::code_pack(code[k], idx, low, high_shift);
    }
}

// rows of odd length (decides whether the unskewed stage applies)
__global__ void __launch_bounds__(kBlock)
k_stream_odd_rows(const uint8_t *__restrict__ len8, uint64_t n, unsigned long long *__restrict__ out) {
    uint32_t c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) c += len8[i] & 1u;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) c += (uint32_t)__shfl_down((int)c, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && c) atomicAdd(out, (unsigned long long)c);  // integer count: exact, order independent
}

// workgroups of k_spmv_stream_xdp<T, DOT, XS, VD> a CU holds.  Both DOT forms are asked about at the first launch of either: the dot-fused
// one is first launched inside the solver's stream capture, where the runtime refuses the query (the fallback of 4 then halved f32's
// grid: 1.74 against 1.45 ms per CG iteration until this was found); a refused query is not remembered.
template <typename T, int XS, int VD> int xdp_resident(bool dot) {
    static std::atomic<int> res[2];  // (relaxed: every thread that asks is told the same, so whose answer stays does not matter)
    if (res[0].load(std::memory_order_relaxed) == 0 || res[1].load(std::memory_order_relaxed) == 0) {
        int a = 0, b = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_spmv_stream_xdp<T, false, XS, VD>, kBlock, 0) == hipSuccess && a > 0)
            res[0].store(a, std::memory_order_relaxed);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_spmv_stream_xdp<T, true, XS, VD>, kBlock, 0) == hipSuccess && b > 0)
            res[1].store(b, std::memory_order_relaxed);
        (void)hipGetLastError();
    }
    const int r = res[dot ? 1 : 0].load(std::memory_order_relaxed);
    return r > 0 ? r : (sizeof(T) == 8 ? 4 : 8);
}

template <typename T>
int launch_xd_t(const T *val, const T *x, T *y, size_t n_rows, T *dot_partials, const uint16_t *scode, const uint32_t *cwin,
                const uint8_t *len8, const uint32_t *tbase, const T *dot_lhs, hipStream_t s, int xs, uint64_t tile_begin, uint64_t tile_end,
                const T *dict, bool dict_high) {
    const uint64_t all_tiles = stream_tiles(n_rows, 1);
    const uint64_t tile0 = tile_begin < all_tiles ? tile_begin : all_tiles, tile1 = tile_end < all_tiles ? tile_end : all_tiles;
    if (tile1 <= tile0) return SMH_OK;
    const uint64_t n_tiles = tile1 - tile0;
    const dim3 grid((unsigned)n_tiles), block(kBlock);
    // K1s XD-V in f64 runs on persistent workgroups (k_spmv_stream_xdp), as many as the chip holds at once.  Measured on C4 (512^3,
    // profiles/r04_k1s_xdv_persistent.log): f64 product 1.45 -> 1.15 ms, CG iteration 3.18 -> 2.99 ms; f32 product 0.73 ms either way
    // (bound by instruction issue, not latency: 8 workgroups per CU already hide the round trips) and its dot-fused form slower
    // (1.76 against 1.52 ms per CG iteration), so f32 keeps one workgroup per tile.  SMH_STREAM_PERSIST = 0 / 1 forces it off / on for both.
    static const int persist_env = getenv("SMH_STREAM_PERSIST") ? atoi(getenv("SMH_STREAM_PERSIST")) : -1;  // tuning knob
    const bool persist = persist_env < 0 ? sizeof(T) == 8 : persist_env != 0;
    if (dict && persist && (xs == 2 || xs == 4)) {
        static std::atomic<int> cus_cache[64];  // (relaxed, as xdp_resident's)
        int dev = 0;
        (void)hipGetDevice(&dev);
        int cus = cus_cache[dev & 63].load(std::memory_order_relaxed);
        if (cus == 0) {
            hipDeviceProp_t prop;
            cus = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
            cus_cache[dev & 63].store(cus, std::memory_order_relaxed);
        }
        static const int per_cu_env = getenv("SMH_STREAM_PERSIST_WGS") ? atoi(getenv("SMH_STREAM_PERSIST_WGS")) : 0;  // tuning knob
#define SMH_XDP(D, P, V)                                                                                                           \
    do {                                                                                                                           \
        const int resident = xdp_resident<T, P, V>(D); /* workgroups of this instantiation one CU holds */                         \
        uint64_t wgx = (uint64_t)(cus / 8 > 0 ? cus / 8 : 1) * (uint64_t)(per_cu_env > 0 ? per_cu_env : resident); /* per XCD */   \
        if (wgx > (n_tiles + 7) / 8) wgx = (n_tiles + 7) / 8;                                                                      \
        if (wgx < 1) wgx = 1;                                                                                                      \
        hipLaunchKernelGGL((k_spmv_stream_xdp<T, D, P, V>), dim3((unsigned)(8 * wgx)), block, 0, s, x, y, (uint64_t)n_rows, n_tiles, \
                           dot_partials, scode, cwin, len8, tbase, dot_lhs, tile0, dict);                                          \
    } while (0)
#define SMH_XDP2(P)                                                                              \
    do {                                                                                         \
        if (dict_high) { if (dot_partials) SMH_XDP(true, P, 2); else SMH_XDP(false, P, 2); }    \
        else { if (dot_partials) SMH_XDP(true, P, 1); else SMH_XDP(false, P, 1); }              \
    } while (0)
        if (xs == 2) SMH_XDP2(2); else SMH_XDP2(4);
#undef SMH_XDP2
#undef SMH_XDP
        SMH_HIP(hipGetLastError());
        return SMH_OK;
    }
#define SMH_XD(D, P, V)                                                                                                              \
    hipLaunchKernelGGL((k_spmv_stream_xd<T, D, P, V>), grid, block, 0, s, val, x, y, (uint64_t)n_rows, n_tiles, dot_partials, scode, \
                       cwin, len8, tbase, dot_lhs, tile0, dict)
#define SMH_XD2(P)                                                                                  \
    do {                                                                                            \
        if (dict && dict_high) { if (dot_partials) SMH_XD(true, P, 2); else SMH_XD(false, P, 2); } \
        else if (dict) { if (dot_partials) SMH_XD(true, P, 1); else SMH_XD(false, P, 1); }         \
        else { if (dot_partials) SMH_XD(true, P, 0); else SMH_XD(false, P, 0); }                   \
    } while (0)
    if (xs == 2) SMH_XD2(2);
    else if (xs == 4) SMH_XD2(4);
    else return fail(SMH_ERR_INVALID, "K1s XD: the stage of x holds 2 or 4 chunks per thread");
#undef SMH_XD2
#undef SMH_XD
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

}  // namespace

// dict != NULL: the codes carry value-dictionary indices (K1s XD-V); val is then not read
int launch_spmv_stream_xd(int dtype, const void *val, const void *x, void *y, size_t n_rows, void *dot_partials, const uint16_t *scode,
                          const uint32_t *cwin, const uint8_t *len8, const uint32_t *tbase, const void *dot_lhs, hipStream_t s, int xs,
                          uint64_t tile_begin, uint64_t tile_end, const void *dict, bool dict_high) {
    if (n_rows == 0) return SMH_OK;
    if (dot_partials && !dot_lhs) dot_lhs = x;  // CG's p.Ap
    if (!dot_partials && !y) return fail(SMH_ERR_INVALID, "K1s: no output");
    if (dtype == SMH_F64)
        return launch_xd_t<double>((const double *)val, (const double *)x, (double *)y, n_rows, (double *)dot_partials, scode, cwin, len8,
                                   tbase, (const double *)dot_lhs, s, xs, tile_begin, tile_end, (const double *)dict, dict_high);
    return launch_xd_t<float>((const float *)val, (const float *)x, (float *)y, n_rows, (float *)dot_partials, scode, cwin, len8, tbase,
                              (const float *)dot_lhs, s, xs, tile_begin, tile_end, (const float *)dict, dict_high);
}

// The dictionary of val's distinct bit patterns: dict_out (device, 32 entries of the value type, sorted by pattern, unused ones zero)
// and *count_out = how many (0: more than 32, or the reserved pattern occurs).  Synchronises the stream.
template <typename T>
static int value_dict_t(const T *val, size_t nnz, T *dict_out, uint32_t *count_out, hipStream_t s) {
    typedef typename XdPat<T>::U U;
    *count_out = 0;
    if (nnz == 0) return SMH_OK;
    uint64_t blocks = (nnz + (uint64_t)kBlock * 64 - 1) / ((uint64_t)kBlock * 64);
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    U *tables = nullptr;
    uint32_t *flags = nullptr;  // [0] overflow, [1] count
    SMH_HIP(hipMalloc((void **)&tables, blocks * kXdDictCap * sizeof(U)));
    hipError_t e = hipMalloc((void **)&flags, 2 * sizeof(uint32_t));
    uint32_t h[2] = {1u, 0u};
    auto go = [&]() -> int {
        SMH_HIP(e);
        SMH_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_value_dict_collect<T>, dim3((unsigned)blocks), dim3(kBlock), 0, s, val, (uint64_t)nnz, tables, flags);
        SMH_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_value_dict_merge<T>, dim3(1), dim3(kBlock), 0, s, (const U *)tables, (uint32_t)blocks, dict_out, flags + 1, flags);
        SMH_HIP(hipGetLastError());
        SMH_HIP(hipMemcpyAsync(h, flags, sizeof h, hipMemcpyDeviceToHost, s));
        SMH_HIP(hipStreamSynchronize(s));
        return SMH_OK;
    };
    const int rc = go();
    (void)hipFree(tables);
    (void)hipFree(flags);
    SMH_TRY(rc);
    *count_out = h[0] ? 0u : h[1];
    return SMH_OK;
}

int stream_value_dict(int dtype, const void *val, size_t nnz, void *dict_out, uint32_t *count_out, hipStream_t s) {
    return dtype == SMH_F64 ? value_dict_t<double>((const double *)val, nnz, (double *)dict_out, count_out, s)
                            : value_dict_t<float>((const float *)val, nnz, (float *)dict_out, count_out, s);
}

// code[k] |= index of val[k] in the dictionary (n entries), in the spare bits of a stage-offset code for a stage of xs * 1024 entries
// do n dictionary entries fit the spare bits ABOVE the offset alone (the cheaper form for the kernel)?
bool stream_value_dict_high(int dtype, uint32_t n, int xs) { return n <= stage::code_values_high((uint32_t)dtype_size(dtype), xs); }

int launch_stream_value_codes(int dtype, const void *val, size_t nnz, const void *dict, uint32_t n, int xs, uint16_t *code, hipStream_t s) {
    if (nnz == 0) return SMH_OK;
    const uint32_t elem = (uint32_t)dtype_size(dtype), high_shift = stage::code_high_shift(elem, xs);
    const uint32_t low = stream_value_dict_high(dtype, n, xs) ? 0u : stage::code_low_bits(elem);  // (low == 0: the whole index goes above the offset)
    uint64_t blocks = (nnz + kBlock - 1) / kBlock;
    if (blocks > 16384) blocks = 16384;
    if (dtype == SMH_F64)
        hipLaunchKernelGGL(k_value_dict_encode<double>, dim3((unsigned)blocks), dim3(kBlock), 0, s, (const double *)val, (uint64_t)nnz, (const double *)dict, n, low, high_shift, code);
    else
        hipLaunchKernelGGL(k_value_dict_encode<float>, dim3((unsigned)blocks), dim3(kBlock), 0, s, (const float *)val, (uint64_t)nnz, (const float *)dict, n, low, high_shift, code);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// how many dictionary entries the spare bits of a code can name, for a stage of xs * 1024 entries
uint32_t stream_value_dict_capacity(int xs) { return stage::code_values(xs); }

int launch_stream_stage_codes(const uint32_t *off, const uint32_t *col, const uint32_t *win, size_t n_rows, uint32_t elem_bytes,
                              uint16_t *code, hipStream_t s) {
    const uint64_t n_tiles = (n_rows + kStreamRows - 1) / kStreamRows;
    if (n_tiles == 0) return SMH_OK;
    const uint64_t blocks = n_tiles < 16384 ? n_tiles : 16384;
    hipLaunchKernelGGL(k_stream_stage_codes, dim3((unsigned)blocks), dim3(kBlock), 0, s, off, col, win, (uint64_t)n_rows, n_tiles, elem_bytes, code);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// *d_out (unsigned long long, device) = rows of odd length among the n_padded byte lengths
int launch_stream_odd_rows(const uint8_t *len8, size_t n_padded, unsigned long long *d_out, hipStream_t s) {
    SMH_HIP(hipMemsetAsync(d_out, 0, sizeof(unsigned long long), s));
    if (n_padded == 0) return SMH_OK;
    uint64_t blocks = (n_padded + kBlock - 1) / kBlock;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_stream_odd_rows, dim3((unsigned)blocks), dim3(kBlock), 0, s, len8, (uint64_t)n_padded, d_out);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

}  // namespace smh
