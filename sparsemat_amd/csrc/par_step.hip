// par_step.hip -- one step of the partitioned path: y = A x on every block and the exchange that makes y the next x.  The two
// exchange backends (RCCL groups; PEER pull kernels ordered by events) and the cross-block folds sit behind ONE seam (par.hpp): a
// step is a list of phases over the seam's parts and never asks which backend runs them.
#include "par.hpp"

#include <cstdlib>

using namespace smh;
using namespace smh::par;

namespace {

constexpr int kMaxPull = 32;  // segments per pull-kernel launch
struct PullArgs {
    const uint32_t *src[kMaxPull];
    uint64_t w0[kMaxPull], w1[kMaxPull];  // 32-bit words [w0, w1) of the full-length buffers
    int n;
};

// dst[w] = src_k[w] for every word w of every segment k: the peers' slices are read where they lie (peer access over
// xGMI; plain device memory when the "peer" block shares the device).  16-byte accesses where both sides allow.
__global__ void __launch_bounds__(kBlock) k_peer_pull(uint32_t *__restrict__ dst, PullArgs a) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (int k = 0; k < a.n; ++k) {
        const uint32_t *__restrict__ src = a.src[k];
        const uint64_t w0 = a.w0[k], w1 = a.w1[k];
        // words [w0, head_end) one by one, [head_end, body_end) as 16-byte pieces, [body_end, w1) one by one.  A word has
        // the same index in both buffers, so the pieces are aligned in both iff the base pointers are equally misaligned.
        uint64_t head_end = w1, body_end = w1;
        const uintptr_t da = reinterpret_cast<uintptr_t>(dst), sa = reinterpret_cast<uintptr_t>(src);
        if (((da ^ sa) & 15u) == 0) {
            const uint64_t mis = (da >> 2) & 3u;  // words by which word 0 is past a 16-byte boundary
            const uint64_t a0 = ((w0 + mis + 3) & ~uint64_t(3)) - mis;
            const uint64_t up = (w1 + mis) & ~uint64_t(3);
            if (up >= mis && a0 < up - mis) { head_end = a0; body_end = up - mis; }
        }
        for (uint64_t w = w0 + tid; w < head_end; w += nthreads) dst[w] = src[w];
        const uint64_t pieces = (body_end - head_end) / 4;
        for (uint64_t q = tid; q < pieces; q += nthreads)
            reinterpret_cast<u32x4 *>(dst + head_end)[q] = reinterpret_cast<const u32x4 *>(src + head_end)[q];
        for (uint64_t w = body_end + tid; w < w1; w += nthreads) dst[w] = src[w];
    }
}

// flag[t] = 1 when a row of the 256-row tile t references a column outside [c0, c1) (the block's own slice of the vector)
__global__ void __launch_bounds__(kBlock) k_par_remote_tiles(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, uint64_t n_rows,
                                                             uint32_t c0, uint32_t c1, uint8_t *__restrict__ flag) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool remote = false;
    if (r < n_rows)
        for (uint64_t k = off[r], e = off[r + 1]; k < e; ++k) {
            const uint32_t c = col[k];
            remote |= c < c0 || c >= c1;
        }
    const bool any = __syncthreads_or(remote);
    if (threadIdx.x == 0) flag[blockIdx.x] = any;
}
static_assert(kTileRows == (size_t)kBlock, "the interior's tiles are the kernel's workgroups");

ncclDataType_t nccl_type(int dtype) { return dtype == SMH_F64 ? ncclDouble : ncclFloat; }

ncclComm_t comm_of(const smh_par *p, const ParBlock &blk) { return p->rank_comm ? p->rank_comm->comm : blk.comm; }

// RCCL backend of a one-process handle: one communicator rank per block, rank id = block id
int ensure_comms(smh_par *p) {
    if (p->comms_ready || p->rank_comm || p->n_blocks <= 1) return SMH_OK;
    size_t i = 0, j = 0;
    if (!distinct_devices(p, &i, &j))
        return fail(SMH_ERR_INVALID, "RCCL backend: blocks %zu and %zu share device %d (one device per block needed; use the PEER backend)", i, j, p->b[i].device);
    std::vector<int> devs(p->b.size());
    for (size_t k = 0; k < p->b.size(); ++k) devs[k] = p->b[k].device;
    std::vector<ncclComm_t> comms(p->b.size(), nullptr);
    SMH_NCCL(ncclCommInitAll(comms.data(), (int)p->b.size(), devs.data()));
    for (size_t k = 0; k < p->b.size(); ++k) p->b[k].comm = comms[k];
    p->comms_ready = true;
    return SMH_OK;
}

// side: on the blocks' exchange streams (sx) instead of their main ones -- the step forks and joins them
hipStream_t xs(const ParBlock &blk, bool side) { return side ? blk.q.sx.get() : blk.q.s.get(); }

// ---- RCCL: the collectives of all local blocks are ONE group issued by the caller (a process per GPU has one block anyway) ------
int exchange_rccl(smh_par *p, smh_par_vec *v, int mode, bool side) {
    SMH_TRY(ensure_comms(p));
    const size_t vs = dtype_size(p->dtype), nb = p->n_blocks, R = p->rows_per_block;
    const ncclDataType_t dt = nccl_type(p->dtype);
    if (mode == SMH_EXCHANGE_ALLGATHER && !p->split.empty()) {
        // blocks of unequal size (a split table): every slice is broadcast from its owner, all of them in ONE group
        SMH_NCCL(ncclGroupStart());
        for (size_t k = 0; k < p->b.size(); ++k) {
            ParBlock &blk = p->b[k];
            SMH_TRY(use(blk));
            for (size_t j = 0; j < nb; ++j) {
                const size_t a = p->split[j], e = p->split[j + 1];
                if (e > a) SMH_NCCL(ncclBroadcast((char *)v->d[k].get() + a * vs, (char *)v->d[k].get() + a * vs, e - a, dt, (int)j, comm_of(p, blk), xs(blk, side)));
            }
        }
        SMH_NCCL(ncclGroupEnd());
        return SMH_OK;
    }
    if (mode == SMH_EXCHANGE_ALLGATHER) {
        // in place: block b's slice already sits at b R of every gathered vector (count R from every rank) ...
        SMH_NCCL(ncclGroupStart());
        for (size_t k = 0; k < p->b.size(); ++k) {
            ParBlock &blk = p->b[k];
            SMH_TRY(use(blk));
            char *buf = (char *)v->d[k].get();
            SMH_NCCL(ncclAllGather(buf + blk.index * R * vs, buf, R, dt, comm_of(p, blk), xs(blk, side)));
        }
        SMH_NCCL(ncclGroupEnd());
        // ... and the last block's remainder rows [n_blocks R, n_rows) follow as one broadcast from their owner
        const size_t rem = p->n_rows - nb * R;
        if (rem) {
            SMH_NCCL(ncclGroupStart());
            for (size_t k = 0; k < p->b.size(); ++k) {
                ParBlock &blk = p->b[k];
                SMH_TRY(use(blk));
                char *tail = (char *)v->d[k].get() + nb * R * vs;
                SMH_NCCL(ncclBroadcast(tail, tail, rem, dt, (int)(nb - 1), comm_of(p, blk), xs(blk, side)));
            }
            SMH_NCCL(ncclGroupEnd());
        }
        return SMH_OK;
    }
    // WINDOW: every piece is a contiguous slice of the vector itself -- sends read the block's own slice, receives land
    // in the peers' slices (disjoint from it): ONE grouped launch of point-to-point operations, no staging, no packing
    SMH_NCCL(ncclGroupStart());
    for (size_t k = 0; k < p->b.size(); ++k) {
        ParBlock &blk = p->b[k];
        SMH_TRY(use(blk));
        char *buf = (char *)v->d[k].get();
        for (size_t q = 0; q < nb; ++q) {
            if (q == blk.index) continue;
            size_t a, e;
            recv_range(part_of(p), blk.index, q, &a, &e);  // what I need of q's slice
            if (a < e) SMH_NCCL(ncclRecv(buf + a * vs, e - a, dt, (int)q, comm_of(p, blk), xs(blk, side)));
            recv_range(part_of(p), q, blk.index, &a, &e);  // what q needs of mine
            if (a < e) SMH_NCCL(ncclSend(buf + a * vs, e - a, dt, (int)q, comm_of(p, blk), xs(blk, side)));
        }
    }
    SMH_NCCL(ncclGroupEnd());
    return SMH_OK;
}

void *slots_rccl(const smh_par *, const ParBlock &blk) { return blk.cg.redv.get(); }

// every block's value of the slot to every block: a 1-element all-gather
int gather_rccl(smh_par *p, int slot) {
    SMH_TRY(ensure_comms(p));
    SMH_NCCL(ncclGroupStart());
    for (ParBlock &blk : p->b) {
        SMH_TRY(use(blk));
        SMH_NCCL(ncclAllGather(fold_mine(p, blk, slot), fold_values(p, blk, slot), 1, nccl_type(p->dtype), comm_of(p, blk), blk.q.s.get()));
    }
    SMH_NCCL(ncclGroupEnd());
    return SMH_OK;
}

// ---- PEER: the exchange in three per-block steps; between two of them every block's calls of the step before must have been
// ISSUED (a wait names an event another block records).  p->pulled is filled by step 2 and read by step 3.
// 1. block k's slice is complete once what its stream holds so far has run
int peer_mark(smh_par *p, size_t k, bool side) {
    ParBlock &blk = p->b[k];
    SMH_TRY(use(blk));
    SMH_HIP(hipEventRecord(blk.q.slice.get(), xs(blk, side)));
    return SMH_OK;
}
// 2. block qi pulls what it needs from the owners' buffers
int peer_pull(smh_par *p, size_t qi, smh_par_vec *v, int mode, bool side) {
    const size_t vs = dtype_size(p->dtype), nl = p->b.size();
    const size_t wpe = vs / 4;  // 32-bit words per entry
    uint8_t *pulled = p->pulled.data();
    ParBlock &q = p->b[qi];
    SMH_TRY(use(q));
    PullArgs args;
    args.n = 0;
    uint64_t words = 0;
    auto flush = [&]() -> int {
        if (args.n == 0) return SMH_OK;
        uint64_t blocks = (words / 4 + kBlock - 1) / kBlock;
        blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
        hipLaunchKernelGGL(k_peer_pull, dim3((unsigned)blocks), dim3(kBlock), 0, xs(q, side), (uint32_t *)v->d[qi].get(), args);
        SMH_HIP(hipGetLastError());
        args.n = 0;
        words = 0;
        return SMH_OK;
    };
    for (size_t si = 0; si < nl; ++si) {
        pulled[qi * nl + si] = 0;
        if (si == qi) continue;
        ParBlock &src = p->b[si];
        size_t a = src.r0, e = src.r1;
        if (mode == SMH_EXCHANGE_WINDOW)
            recv_range(part_of(p), q.index, src.index, &a, &e);
        if (a >= e) continue;
        pulled[qi * nl + si] = 1;
        SMH_HIP(hipStreamWaitEvent(xs(q, side), src.q.slice.get(), 0));
        if (p->peer_ok[qi * nl + si]) {
            args.src[args.n] = (const uint32_t *)v->d[si].get();
            args.w0[args.n] = (uint64_t)a * wpe;
            args.w1[args.n] = (uint64_t)e * wpe;
            words += (uint64_t)(e - a) * wpe;
            if (++args.n == kMaxPull) SMH_TRY(flush());
        } else {  // no direct access between the two devices: the runtime stages the copy
            SMH_HIP(hipMemcpyPeerAsync((char *)v->d[qi].get() + a * vs, q.device, (const char *)v->d[si].get() + a * vs, src.device, (e - a) * vs, xs(q, side)));
        }
    }
    SMH_TRY(flush());
    SMH_HIP(hipEventRecord(q.q.done.get(), xs(q, side)));
    return SMH_OK;
}
// 3. block si does not overwrite its slice while a peer may still be reading it
int peer_guard(smh_par *p, size_t si, bool side) {
    const size_t nl = p->b.size();
    ParBlock &src = p->b[si];
    SMH_TRY(use(src));
    for (size_t qi = 0; qi < nl; ++qi)
        if (p->pulled[qi * nl + si]) SMH_HIP(hipStreamWaitEvent(xs(src, side), p->b[qi].q.done.get(), 0));
    return SMH_OK;
}

void *slots_peer(const smh_par *p, const ParBlock &) { return p->h_red.get(); }

// A fold's meeting in three steps (each needs the step before ISSUED by every block it names): every block's value is written ->
// every block may read all of them.  Through ONE meeting point (block 0's stream waits for the others' records, the others wait for
// its record after that): 2 (n - 1) waits instead of n (n - 1)
int red_mark(smh_par *p, size_t k, int slot) {  // block k's value of the slot is written once its stream gets here
    ParBlock &blk = p->b[k];
    SMH_TRY(use(blk));
    SMH_HIP(hipEventRecord(blk.q.red[slot].get(), blk.q.s.get()));
    return SMH_OK;
}
int red_hub(smh_par *p, int slot) {  // block 0's stream has seen them all
    ParBlock &hub = p->b[0];
    SMH_TRY(use(hub));
    for (size_t k = 1; k < p->b.size(); ++k) SMH_HIP(hipStreamWaitEvent(hub.q.s.get(), p->b[k].q.red[slot].get(), 0));
    if (p->b.size() > 1) SMH_HIP(hipEventRecord(hub.q.all[slot].get(), hub.q.s.get()));
    return SMH_OK;
}
int red_wait(smh_par *p, size_t k, int slot) {  // ... and block k's waits for that
    if (k == 0) return SMH_OK;
    SMH_TRY(use(p->b[k]));
    SMH_HIP(hipStreamWaitEvent(p->b[k].q.s.get(), p->b[0].q.all[slot].get(), 0));
    return SMH_OK;
}

// ---- the seam: the two backends as the same seven parts (NULL: the backend has nothing to do there) -----------------------------
struct Backend {
    int (*begin)(smh_par *, size_t, bool);
    int (*all)(smh_par *, smh_par_vec *, int, bool);
    int (*pull)(smh_par *, size_t, smh_par_vec *, int, bool);
    int (*end)(smh_par *, size_t, bool);
    int (*put)(smh_par *, size_t, int);
    int (*meet)(smh_par *, int);
    int (*get)(smh_par *, size_t, int);
    void *(*slots)(const smh_par *, const ParBlock &);  // 2 x n_blocks values: the fold slots as a block's kernels address them
};
const Backend kPeer = {peer_mark, nullptr, peer_pull, peer_guard, red_mark, red_hub, red_wait, slots_peer};
const Backend kRccl = {nullptr, exchange_rccl, nullptr, nullptr, nullptr, gather_rccl, nullptr, slots_rccl};
const Backend &backend(const smh_par *p) { return p->backend == SMH_PAR_BACKEND_RCCL ? kRccl : kPeer; }

}  // namespace

namespace smh {
namespace par {

// (an exchange part does nothing when the mode is NONE, a fold part nothing for a lone block, either nothing where the backend has no such part)
static bool moves(int mode) { return mode != SMH_EXCHANGE_NONE; }
int xchg_begin(smh_par *p, size_t k, int mode, bool side) { return moves(mode) && backend(p).begin ? backend(p).begin(p, k, side) : SMH_OK; }
int xchg_all(smh_par *p, smh_par_vec *v, int mode, bool side) { return moves(mode) && backend(p).all ? backend(p).all(p, v, mode, side) : SMH_OK; }
int xchg_pull(smh_par *p, size_t k, smh_par_vec *v, int mode, bool side) { return moves(mode) && backend(p).pull ? backend(p).pull(p, k, v, mode, side) : SMH_OK; }
int xchg_end(smh_par *p, size_t k, int mode, bool side) { return moves(mode) && backend(p).end ? backend(p).end(p, k, side) : SMH_OK; }
int fold_put(smh_par *p, size_t k, int slot) { return !lone_block_skips(p) && backend(p).put ? backend(p).put(p, k, slot) : SMH_OK; }
int fold_all(smh_par *p, int slot) { return !lone_block_skips(p) && backend(p).meet ? backend(p).meet(p, slot) : SMH_OK; }
int fold_get(smh_par *p, size_t k, int slot) { return !lone_block_skips(p) && backend(p).get ? backend(p).get(p, k, slot) : SMH_OK; }
void *fold_values(const smh_par *p, const ParBlock &blk, int slot) {
    return (char *)backend(p).slots(p, blk) + (size_t)slot * p->n_blocks * dtype_size(p->dtype);
}
void *fold_mine(const smh_par *p, const ParBlock &blk, int slot) { return (char *)fold_values(p, blk, slot) + blk.index * dtype_size(p->dtype); }

// One block has nobody to exchange with.  SMH_PAR_EXCHANGE_SINGLE=1 (test knob) still sends a lone RANK through the RCCL
// calls -- an in-place all-gather of one rank, an empty send/receive group, the 1-element gathers of the folds -- so that
// a one-GPU box executes the very call sequence the ranks of a node run.
bool lone_block_skips(const smh_par *p) {
    if (p->n_blocks > 1) return false;
    static const bool forced = getenv("SMH_PAR_EXCHANGE_SINGLE") && atoi(getenv("SMH_PAR_EXCHANGE_SINGLE")) != 0;
    return !(forced && p->rank_comm);
}

int resolve_mode(const smh_par *p, int mode, int *out) {
    if (mode < SMH_EXCHANGE_NONE || mode > SMH_EXCHANGE_AUTO) return fail(SMH_ERR_INVALID, "unknown exchange mode %d", mode);
    if (lone_block_skips(p)) { *out = SMH_EXCHANGE_NONE; return SMH_OK; }
    if (p->n_blocks <= 1) { *out = mode == SMH_EXCHANGE_AUTO ? SMH_EXCHANGE_ALLGATHER : mode; return SMH_OK; }
    if (mode == SMH_EXCHANGE_AUTO) {
        int m = SMH_EXCHANGE_ALLGATHER;
        // a window is addressed by column AND owned by row: only meaningful when the vector is both (square matrix)
        if (p->n_rows == p->n_cols) plan_summary(part_of(p), &m, nullptr);
        *out = m;
        return SMH_OK;
    }
    if (mode == SMH_EXCHANGE_WINDOW && p->n_rows != p->n_cols)
        return fail(SMH_ERR_INVALID, "a window exchange needs a square matrix (%zu x %zu)", p->n_rows, p->n_cols);
    *out = mode;
    return SMH_OK;
}

// is every local block on a device of its own?  (*i, *j, optional: the first two blocks that share one)
bool distinct_devices(const smh_par *p, size_t *i, size_t *j) {
    for (size_t a = 0; a < p->b.size(); ++a)
        for (size_t c = a + 1; c < p->b.size(); ++c)
            if (p->b[a].device == p->b[c].device) {
                if (i) { *i = a; *j = c; }
                return false;
            }
    return true;
}

int exchange(smh_par *p, smh_par_vec *v, int mode, bool side) {
    int m = SMH_EXCHANGE_NONE;
    SMH_TRY(resolve_mode(p, mode, &m));
    if (m == SMH_EXCHANGE_NONE) return SMH_OK;
    if (v->n != p->n_rows)
        return fail(SMH_ERR_DIM_MISMATCH, "exchange: the vector has %zu entries, the partition owns %zu rows", v->n, p->n_rows);
    SMH_TRY(par_for(p, [&](size_t k) { return xchg_begin(p, k, m, side); }));
    SMH_TRY(xchg_all(p, v, m, side));
    SMH_TRY(par_for(p, [&](size_t k) { return xchg_pull(p, k, v, m, side); }));
    return par_for(p, [&](size_t k) { return xchg_end(p, k, m, side); });
}

// after every local block wrote fold_mine(slot): make all n_blocks values visible to every block's stream
int combine(smh_par *p, int slot) {
    SMH_TRY(par_for(p, [&](size_t k) { return fold_put(p, k, slot); }));
    SMH_TRY(fold_all(p, slot));
    return par_for(p, [&](size_t k) { return fold_get(p, k, slot); });
}

// ---- the exchange beside the product ("overlap the gather with the next block of rows") ----------------------
// The blocks are independent (sparsemat_par.rs:54-64: every block multiplies on its own, results at b R), so WHICH of a block's
// rows are multiplied first is free of semantics.  A WINDOW exchange moves only what blocks reference of each other; a block's
// interior rows [in0, in1) neither feed it nor need it.  So the exchange runs on a second stream per block while the interior
// rows are multiplied: fork after what the exchange reads is written, join before what it writes is read.
int fork_one(ParBlock &blk) {
    SMH_TRY(use(blk));
    SMH_HIP(hipEventRecord(blk.q.fork.get(), blk.q.s.get()));
    SMH_HIP(hipStreamWaitEvent(blk.q.sx.get(), blk.q.fork.get(), 0));
    return SMH_OK;
}
int join_one(ParBlock &blk) {
    SMH_TRY(use(blk));
    SMH_HIP(hipEventRecord(blk.q.join.get(), blk.q.sx.get()));
    SMH_HIP(hipStreamWaitEvent(blk.q.s.get(), blk.q.join.get(), 0));
    return SMH_OK;
}

// the interior of a block as ITS kernel for `variant` can launch it: [*a, *e) (local rows; *a == *e: the product is not split)
int interior_for(ParBlock &blk, int variant, size_t *a, size_t *e) {
    *a = *e = 0;
    if (blk.in1 <= blk.in0) return SMH_OK;
    size_t gran = 0;
    SMH_TRY(spmv_rows_granularity(blk.m, variant, &gran));
    round_interior(blk.in0, blk.in1, blk.r1 - blk.r0, gran, a, e);
    return SMH_OK;
}

// does a window exchange run beside the products for this call?  (every local block decides the same way: the mode is global)
bool overlapped(const smh_par *p, int resolved_mode) {
    static const bool off = getenv("SMH_PAR_OVERLAP") && atoi(getenv("SMH_PAR_OVERLAP")) == 0;  // tuning knob
    return p->overlap && !off && resolved_mode == SMH_EXCHANGE_WINDOW && !lone_block_skips(p);
}

// a block's interior: the largest run of 256-row tiles that holds no row another block references and no row that references
// another block's columns (square matrices: the window exchange's precondition)
int find_interiors(smh_par *p) {
    const size_t nb = p->n_blocks;
    for (ParBlock &blk : p->b) {
        blk.in0 = blk.in1 = 0;
        const size_t n_loc = blk.r1 - blk.r0;
        if (p->n_rows != p->n_cols || n_loc == 0 || nb <= 1) continue;
        SMH_TRY(use(blk));
        const size_t n_tiles = (n_loc + kTileRows - 1) / kTileRows;
        std::vector<uint8_t> dirty(n_tiles, 0);
        if (smh_crs_nnz(blk.m)) {
            DevArray<uint8_t> flag;
            SMH_TRY(flag.alloc(n_tiles));
            hipLaunchKernelGGL(k_par_remote_tiles, dim3((unsigned)n_tiles), dim3(kBlock), 0, blk.q.s.get(), blk.m->d_off, blk.m->d_col, (uint64_t)n_loc,
                               (uint32_t)blk.r0, (uint32_t)blk.r1, flag.get());
            SMH_HIP(hipGetLastError());
            SMH_HIP(hipMemcpyAsync(dirty.data(), flag.get(), n_tiles, hipMemcpyDeviceToHost, blk.q.s.get()));
            SMH_HIP(hipStreamSynchronize(blk.q.s.get()));
        }
        mark_referenced_tiles(part_of(p), blk.index, blk.r0, dirty.data());
        size_t t0, t1;
        longest_clean_run(dirty.data(), n_tiles, &t0, &t1);
        blk.in0 = t0 * kTileRows;
        blk.in1 = t1 * kTileRows < n_loc ? t1 * kTileRows : n_loc;
        if (blk.in1 <= blk.in0) blk.in0 = blk.in1 = 0;
    }
    return SMH_OK;
}

}  // namespace par
}  // namespace smh

extern "C" {

// ---- y = A x, device resident ---------------------------------------------------------------------------------------------
int smh_par_spmv_dev(smh_par *p, const smh_par_vec *x, smh_par_vec *y, int variant, int mode) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(check_vec(p, x, "x"));
    SMH_TRY(check_vec(p, y, "y"));
    if (x == y) return fail(SMH_ERR_INVALID, "x and y must be different vectors");
    if (y->n != p->n_rows) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    const size_t vs = dtype_size(p->dtype);
    int m = SMH_EXCHANGE_NONE;
    SMH_TRY(resolve_mode(p, mode, &m));
    if (!overlapped(p, m))
        return issue(p, [&]() -> int {
            SMH_TRY(par_for(p, [&](size_t k) -> int {
                ParBlock &blk = p->b[k];
                SMH_TRY(use(blk));
                return smh_crs_spmv_dev(blk.m, x->d[k].get(), x->n, (char *)y->d[k].get() + blk.r0 * vs, variant, blk.q.s.get());  // results at b R (:64)
            }));
            return exchange(p, y, mode);
        });
    // the rows other blocks reference and their exchange on the side streams, the interior rows on the main ones -- BOTH from the start:
    // the boundary rows are one or two launches of a few workgroups (13 us each on an otherwise idle chip: 27 us of a 355 us step when
    // they ran ahead of everything, profiles/r04_par_boundary_on_side_stream.log)
    std::vector<size_t> ia(p->b.size(), 0), ie(p->b.size(), 0);
    return issue(p, [&]() -> int {
        SMH_TRY(par_for(p, [&](size_t k) -> int {
            ParBlock &blk = p->b[k];
            SMH_TRY(use(blk));
            SMH_TRY(interior_for(blk, variant, &ia[k], &ie[k]));
            char *yk = (char *)y->d[k].get() + blk.r0 * vs;
            if (ie[k] > ia[k]) {
                SMH_TRY(fork_one(blk));  // (the side stream after everything the main one holds: x is written, y's readers are through)
                SMH_TRY(spmv_enqueue_rows_short(blk.m, x->d[k].get(), x->n, yk, variant, blk.q.sx.get(), 0, ia[k]));
                SMH_TRY(spmv_enqueue_rows_short(blk.m, x->d[k].get(), x->n, yk, variant, blk.q.sx.get(), ie[k], blk.r1 - blk.r0));
            } else {
                SMH_TRY(smh_crs_spmv_dev(blk.m, x->d[k].get(), x->n, yk, variant, blk.q.s.get()));
                SMH_TRY(fork_one(blk));
            }
            return xchg_begin(p, k, m, true);
        }));
        SMH_TRY(xchg_all(p, y, m, true));
        SMH_TRY(par_for(p, [&](size_t k) -> int {
            SMH_TRY(xchg_pull(p, k, y, m, true));
            ParBlock &blk = p->b[k];
            if (ie[k] <= ia[k]) return SMH_OK;
            SMH_TRY(use(blk));
            return spmv_enqueue_rows(blk.m, x->d[k].get(), x->n, (char *)y->d[k].get() + blk.r0 * vs, variant, blk.q.s.get(), ia[k], ie[k]);
        }));
        return par_for(p, [&](size_t k) -> int {
            SMH_TRY(xchg_end(p, k, m, true));
            return join_one(p->b[k]);
        });
    });
}

int smh_par_set_overlap(smh_par *p, int on) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL handle");
    DeviceGuard g;
    SMH_TRY(sync_all(p));
    p->overlap = on != 0;
    return SMH_OK;
}

int smh_par_interior(const smh_par *p, size_t local_block, int variant, size_t *row_begin, size_t *row_end) {
    if (!p || local_block >= p->b.size() || !row_begin || !row_end) return fail(SMH_ERR_INVALID, "bad argument");
    DeviceGuard g;
    ParBlock &blk = const_cast<smh_par *>(p)->b[local_block];
    SMH_TRY(use(blk));
    return interior_for(blk, variant, row_begin, row_end);
}

int smh_par_exchange(smh_par *p, smh_par_vec *v, int mode) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(check_vec(p, v, "vector"));
    return issue(p, [&] { return exchange(p, v, mode); });
}

// y[0..n_rows) = A x on host vectors: every block gets the part of x its columns reference, all blocks run concurrently
int smh_par_spmv(smh_par *p, const void *x_host, size_t x_len, void *y_host, int variant) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL handle");
    if (p->rank_comm) return fail(SMH_ERR_INVALID, "smh_par_spmv takes whole host vectors: one-process handles only (use smh_par_spmv_dev)");
    if (!y_host || (x_len && !x_host)) return fail(SMH_ERR_INVALID, "NULL host vector");
    const size_t vs = dtype_size(p->dtype);
    return issue(p, [&]() -> int {
        for (ParBlock &blk : p->b) {
            SMH_TRY(use(blk));
            if (!blk.io.built) {
                HostStaging st;  // (both arrays or neither)
                SMH_TRY(st.x.alloc((p->n_cols ? p->n_cols : 1) * vs));
                SMH_TRY(st.y.alloc((blk.r1 > blk.r0 ? blk.r1 - blk.r0 : 1) * vs));
                st.built = true;
                blk.io = std::move(st);
            }
            if (p->needs[blk.index]) {
                const uint32_t lo = p->lo[blk.index], hi = p->hi[blk.index];
                if ((size_t)hi >= x_len)  // rhs.get(j): densevec.rs:41
                    return fail(SMH_ERR_INDEX_RANGE, "index out of bounds: the len is %zu but the index is %u", x_len, hi);
                SMH_HIP(hipMemcpyAsync((char *)blk.io.x.get() + (size_t)lo * vs, (const char *)x_host + (size_t)lo * vs, ((size_t)hi - lo + 1) * vs,
                                       hipMemcpyHostToDevice, blk.q.s.get()));
            }
            SMH_TRY(smh_crs_spmv_dev(blk.m, blk.io.x.get(), x_len < p->n_cols ? x_len : p->n_cols, blk.io.y.get(), variant, blk.q.s.get()));
            if (blk.r1 > blk.r0)
                SMH_HIP(hipMemcpyAsync((char *)y_host + blk.r0 * vs, blk.io.y.get(), (blk.r1 - blk.r0) * vs, hipMemcpyDeviceToHost, blk.q.s.get()));
        }
        return sync_all(p);
    });
}

}  // extern "C"
