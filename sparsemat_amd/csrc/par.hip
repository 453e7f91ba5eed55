// par.hip -- SparseMatPar<SparseMatCRS<T,u32>> behind the C ABI: row blocks on the GPUs of one node, the exchange of
// the dense vector INSIDE the library (RCCL over xGMI, or direct peer reads), device-resident CG.
// This unit: communicators, construction and destruction, accessors, distributed vectors.  The product step, the exchange and the
// backends are par_step.hip, the solver is par_cg.hip, the partition's arithmetic par_plan.hpp, the issuing threads par_issue.hpp;
// par.hpp holds what they share.
//
// Reference (sparsemat_par.rs:12-35, 86-107): n_blocks sub-matrices of R = max_n_rows / n_blocks local rows each, block b
// owning the global rows [b R, (b+1) R) with local row ids and GLOBAL column ids; `mvp` is the serial trait default
// walking iter_row(row) -> sub_matrices[block].iter_row(local).  Its commented-out mvp_par (:37-68) is the design these
// files complete: every block multiplies against the shared rhs, the results go to offset b * R, the pieces are
// gathered.  get_block_and_row_id clamps the block id to n_blocks (:32) -- one past the last block -- so a row beyond
// n_blocks R panics; here, as SURVEY 8b prescribes, the LAST block takes the remainder (clamp to n_blocks - 1).
//
// Device formulation.  Block b is an ordinary smh_crs on its device (all kernel families apply) with a stream of its
// own.  A distributed vector (smh_par_vec) is one FULL-LENGTH buffer per local block; block b owns [b R, (b+1) R) of it.
// y = A x: every block writes its slice of y, then ONE exchange makes y usable as the next x:
//   ALLGATHER  in-place ncclAllGather at recvbuff + b R (+ ncclBroadcast of a ragged last block's tail)
//   WINDOW     block q receives exactly [lo_q, hi_q] \ own slice (its column interval, a create-time statistic):
//              grouped ncclSend / ncclRecv on slices of the vector itself -- a banded matrix moves a halo
// Backends: RCCL (ncclCommInitAll over the blocks' devices in one process; ncclCommInitRank with one process per GPU,
// smh_comm_*), or PEER for a one-process handle: one pull kernel per block reads the peers' slices straight through
// peer access (all xGMI links of the destination at once; hipMemcpyPeerAsync where peer access is unavailable).  PEER is
// also what runs when several blocks share a device, which is how the whole path -- partition, plans, exchanges, folds,
// solver -- is exercised on a one-GPU box.  A step is a list of phases over the parts both backends have (the seam, par.hpp).
#include "par.hpp"

#include <cstdlib>
#include <cstring>

using namespace smh;
using namespace smh::par;

namespace smh {
namespace par {

int use(const ParBlock &blk) {
    // (called before every runtime call of a block; a thread that already is on the block's device -- always, when the blocks share
    // one -- skips the runtime's device switch)
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == blk.device) return SMH_OK;
    SMH_HIP(hipSetDevice(blk.device));
    return SMH_OK;
}

int sync_all(smh_par *p) {
    for (ParBlock &blk : p->b) {
        SMH_TRY(use(blk));
        SMH_HIP(hipStreamSynchronize(blk.q.s.get()));
        if (blk.q.sx.get()) SMH_HIP(hipStreamSynchronize(blk.q.sx.get()));
    }
    return SMH_OK;
}

bool threads_wanted(const smh_par *p) {
    if (p->b.size() < 2) return false;
    if (p->use_threads >= 0) return p->use_threads != 0;
    // automatic = OFF: measured with 8 blocks on one device (the only multi-block set-up this build has had), the runtime serialises
    // its callers -- 8 threads issue an iteration of the solver in 0.37 ms where one thread takes 0.47 ms, and the interleaving they
    // produce costs the device more than that saves (0.59 against 0.475 ms per iteration, profiles/r04_par_cg_threads.log).  On a
    // node, a device per block, the runtime's per-device queues may make it pay: SMH_PAR_THREADS=1 / smh_par_set_threads(p, 1)
    static const bool on = getenv("SMH_PAR_THREADS") && atoi(getenv("SMH_PAR_THREADS")) != 0;  // tuning knob
    return on;
}

int vec_create(smh_par *p, size_t n, smh_par_vec **out) {
    const size_t vs = dtype_size(p->dtype);
    std::vector<DevArray<char>> d(p->b.size());  // (an early return frees what it holds)
    for (size_t k = 0; k < p->b.size(); ++k) {
        SMH_TRY(use(p->b[k]));
        SMH_TRY(d[k].alloc((n ? n : 1) * vs));
        SMH_HIP(hipMemsetAsync(d[k].get(), 0, (n ? n : 1) * vs, p->b[k].q.s.get()));
    }
    smh_par_vec *v = new (std::nothrow) smh_par_vec();
    if (!v) return fail(SMH_ERR_OOM, "host allocation failed");
    v->p = p; v->n = n; v->d = std::move(d);
    *out = v;
    return SMH_OK;
}

void vec_destroy(smh_par_vec *v) {
    if (!v) return;
    for (size_t k = 0; k < v->d.size(); ++k) {
        (void)hipSetDevice(v->p->b[k].device);
        (void)hipStreamSynchronize(v->p->b[k].q.s.get());
        v->d[k].reset();
    }
    (void)hipGetLastError();
    delete v;
}

int check_vec(const smh_par *p, const smh_par_vec *v, const char *what) {
    if (!v) return fail(SMH_ERR_INVALID, "NULL %s", what);
    if (v->p != p) return fail(SMH_ERR_INVALID, "%s belongs to another partition", what);
    return SMH_OK;
}

}  // namespace par
}  // namespace smh

namespace {

// streams, events, peer access, the table of column intervals, the backend: everything after the blocks exist
int finish_par(smh_par *p) {
    const size_t nl = p->b.size();
    for (ParBlock &blk : p->b) {
        SMH_TRY(use(blk));
        SMH_TRY(blk.q.s.create());
        SMH_TRY(blk.q.sx.create());
        for (Event *e : {&blk.q.fork, &blk.q.join, &blk.q.slice, &blk.q.done, &blk.q.red[0], &blk.q.red[1], &blk.q.all[0], &blk.q.all[1]}) SMH_TRY(e->create());
    }
    // direct device-to-device reads where the hardware offers them (xGMI)
    p->peer_ok.assign(nl * nl, 0);
    p->pulled.assign(nl * nl, 0);
    for (size_t a = 0; a < nl; ++a)
        for (size_t c = 0; c < nl; ++c) {
            if (p->b[a].device == p->b[c].device) { p->peer_ok[a * nl + c] = 1; continue; }
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, p->b[a].device, p->b[c].device) == hipSuccess && can) {
                (void)hipSetDevice(p->b[a].device);
                const hipError_t e = hipDeviceEnablePeerAccess(p->b[c].device, 0);
                if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) p->peer_ok[a * nl + c] = 1;
            }
            (void)hipGetLastError();
        }
    const bool distinct = distinct_devices(p);
    if (p->rank_comm) {
        p->backend = SMH_PAR_BACKEND_RCCL;
    } else {
        p->backend = distinct && nl > 1 ? SMH_PAR_BACKEND_RCCL : SMH_PAR_BACKEND_PEER;
        if (const char *e = getenv("SMH_PAR_BACKEND")) {
            if (!strcmp(e, "peer")) p->backend = SMH_PAR_BACKEND_PEER;
            else if (!strcmp(e, "rccl") && distinct) p->backend = SMH_PAR_BACKEND_RCCL;
        }
    }
    return SMH_OK;
}

int own_interval(ParBlock &blk, size_t n_cols, uint8_t *needs, uint32_t *lo, uint32_t *hi) {
    *needs = smh_crs_nnz(blk.m) != 0;
    SMH_TRY(smh_crs_col_range(blk.m, lo, hi));
    if (*needs && (size_t)*hi >= n_cols)
        return fail(SMH_ERR_INDEX_RANGE, "block %zu: column %u out of range for %zu columns", blk.index, *hi, n_cols);
    return SMH_OK;
}

// a split table's rules (par_plan.hpp), in words
int split_ok(size_t n_blocks, size_t n_rows, const size_t *split) {
    size_t k = 0;
    switch (check_split(n_blocks, n_rows, split, &k)) {
    case SplitFault::Ends: return fail(SMH_ERR_INVALID, "split table: must run from 0 to n_rows (%zu)", n_rows);
    case SplitFault::Descends: return fail(SMH_ERR_INVALID, "split table: block %zu ends before it begins", k);
    case SplitFault::None: break;
    }
    return SMH_OK;
}

// What the three constructors share: the partition's arithmetic checked, a handle with its common fields and n_local blocks, the caller's fill step
// (the blocks, their column intervals, finish_par), the interiors; a handle that failed is destroyed with the error text kept, the device restored.
template <class Fill>
int make_par(int dtype, size_t n_blocks, size_t n_local, size_t n_rows, size_t n_cols, smh_comm *rank_comm, Fill &&fill, smh_par **out) {
    if (n_blocks == 0) return fail(SMH_ERR_INVALID, "SparseMatPar needs at least one block");
    const size_t rpb = n_rows / n_blocks;  // sparsemat_par.rs:21
    if (rpb == 0) return fail(SMH_ERR_INVALID, "fewer rows (%zu) than blocks (%zu): rows per block would be 0 (sparsemat_par.rs:21,32)", n_rows, n_blocks);
    DeviceGuard g;
    smh_par *p = new (std::nothrow) smh_par();
    if (!p) return fail(SMH_ERR_OOM, "host allocation failed");
    p->dtype = dtype; p->n_rows = n_rows; p->n_cols = n_cols; p->rows_per_block = rpb; p->n_blocks = n_blocks; p->rank_comm = rank_comm;
    p->b.resize(n_local);
    p->lo.assign(n_blocks, 0); p->hi.assign(n_blocks, 0); p->needs.assign(n_blocks, 0);
    // an issuing thread lives on its block's device, hands its error text to the caller, and an exception out of it is a status
    p->pool.hooks.start = [](void *ctx, size_t k) { (void)hipSetDevice(static_cast<smh_par *>(ctx)->b[k].device); };
    p->pool.hooks.message = smh_last_error;
    p->pool.hooks.ctx = p;
    p->pool.hooks.thrown = SMH_ERR_OOM;
    int rc = fill(p);
    if (rc == SMH_OK) rc = find_interiors(p);
    if (rc != SMH_OK) return keep_error(rc, [&] { smh_par_destroy(p); });
    *out = p;
    return SMH_OK;
}

}  // namespace

extern "C" {

// ---- one rank of an RCCL communicator (one process per GPU) ----------------------------------------------------------
int smh_comm_unique_id(void *id_out) {
    if (!id_out) return fail(SMH_ERR_INVALID, "NULL id buffer");
    static_assert(sizeof(ncclUniqueId) == SMH_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    SMH_NCCL(ncclGetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return SMH_OK;
}

int smh_comm_create(const void *id, int n_ranks, int rank, smh_comm **out) {
    if (!id || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(SMH_ERR_INVALID, "rank %d of %d", rank, n_ranks);
    SMH_TRY(require_device());
    smh_comm *c = new (std::nothrow) smh_comm();
    if (!c) return fail(SMH_ERR_OOM, "host allocation failed");
    c->n_ranks = n_ranks;
    c->rank = rank;
    c->device = current_device();
    auto go = [&]() -> int {
        ncclUniqueId uid;
        memcpy(&uid, id, sizeof uid);
        SMH_NCCL(ncclCommInitRank(&c->comm, n_ranks, uid, rank));
        SMH_TRY(c->s.create());
        // (the ranks' plan table is gathered here: a rank must not be able to fail between its local checks and that collective)
        const size_t table = kPlanWords * sizeof(uint32_t) * (size_t)n_ranks;
        SMH_TRY(c->d_scratch.alloc(table > 64 ? table : 64));
        return SMH_OK;
    };
    const int rc = go();
    if (rc != SMH_OK) return keep_error(rc, [&] { smh_comm_destroy(c); });
    *out = c;
    return SMH_OK;
}

int smh_comm_destroy(smh_comm *c) {
    if (!c) return SMH_OK;
    DeviceGuard g;
    (void)hipSetDevice(c->device);
    if (c->s.get()) (void)hipStreamSynchronize(c->s.get());
    c->s = Stream();
    if (c->comm) (void)ncclCommDestroy(c->comm);
    delete c;  // (its scratch)
    (void)hipGetLastError();
    return SMH_OK;
}

int smh_comm_size(const smh_comm *c) { return c ? c->n_ranks : 0; }
int smh_comm_rank(const smh_comm *c) { return c ? c->rank : -1; }

int smh_comm_ranks_seen(const smh_comm *c, int *count_out, int *device_out) {
    if (!c || !c->comm) return fail(SMH_ERR_INVALID, "NULL communicator");
    if (count_out) SMH_NCCL(ncclCommCount(c->comm, count_out));
    if (device_out) SMH_NCCL(ncclCommCuDevice(c->comm, device_out));
    return SMH_OK;
}

int smh_rccl_version(int *version_out) {
    if (!version_out) return fail(SMH_ERR_INVALID, "NULL argument");
    SMH_NCCL(ncclGetVersion(version_out));
    return SMH_OK;
}

int smh_comm_max_f64(smh_comm *c, double *value_inout) {
    if (!c || !value_inout) return fail(SMH_ERR_INVALID, "NULL argument");
    DeviceGuard g;
    SMH_HIP(hipSetDevice(c->device));
    SMH_HIP(hipMemcpyAsync(c->d_scratch.get(), value_inout, sizeof(double), hipMemcpyHostToDevice, c->s.get()));
    SMH_NCCL(ncclAllReduce(c->d_scratch.get(), c->d_scratch.get(), 1, ncclDouble, ncclMax, c->comm, c->s.get()));
    SMH_HIP(hipMemcpyAsync(value_inout, c->d_scratch.get(), sizeof(double), hipMemcpyDeviceToHost, c->s.get()));
    SMH_HIP(hipStreamSynchronize(c->s.get()));
    return SMH_OK;
}

int smh_comm_barrier(smh_comm *c) {
    if (!c) return fail(SMH_ERR_INVALID, "NULL communicator");
    DeviceGuard g;
    SMH_HIP(hipSetDevice(c->device));
    SMH_HIP(hipDeviceSynchronize());  // this rank's device work first: the barrier then orders the ranks' host timelines
    double one = 1.0;
    return smh_comm_max_f64(c, &one);
}

// ---- construction ----------------------------------------------------------------------------------------------------
int smh_par_create(smh_dtype dtype, size_t n_blocks, const int *device_ids, size_t n_rows, size_t n_cols,
                   const uint32_t *offset_rows, const uint32_t *columns, const void *values, int validate, smh_par **out) {
    return smh_par_create_split(dtype, n_blocks, device_ids, n_rows, n_cols, offset_rows, columns, values, validate, SMH_SPLIT_ROWS, out);
}

int smh_par_create_split(smh_dtype dtype, size_t n_blocks, const int *device_ids, size_t n_rows, size_t n_cols,
                         const uint32_t *offset_rows, const uint32_t *columns, const void *values, int validate, int split_mode, smh_par **out) {
    if (!out) return fail(SMH_ERR_INVALID, "NULL out pointer");
    if (split_mode != SMH_SPLIT_ROWS && split_mode != SMH_SPLIT_NNZ) return fail(SMH_ERR_INVALID, "unknown split mode %d", split_mode);
    if (dtype != SMH_F32 && dtype != SMH_F64) return fail(SMH_ERR_INVALID, "unknown dtype %d", (int)dtype);
    if (n_blocks && !offset_rows) return fail(SMH_ERR_INVALID, "NULL offset_rows");  // (no block at all: make_par's message)
    const size_t vs = dtype_size(dtype);
    return make_par(dtype, n_blocks, n_blocks, n_rows, n_cols, nullptr, [&](smh_par *p) -> int {
        int n_dev = 0;
        SMH_TRY(smh_device_count(&n_dev));
        if (n_dev == 0) return fail(SMH_ERR_NO_DEVICE, "no HIP device visible: libsparsemat_hip has no CPU fallback");
        if (split_mode == SMH_SPLIT_NNZ) split_by_nnz(n_blocks, n_rows, offset_rows, p->split);
        std::vector<uint32_t> off;
        for (size_t k = 0; k < n_blocks; ++k) {
            ParBlock &blk = p->b[k];
            blk.index = k;
            blk.device = device_ids ? device_ids[k] : (int)(k % (size_t)n_dev);
            if (blk.device < 0 || blk.device >= n_dev) return fail(SMH_ERR_INVALID, "block %zu: device %d of %d", k, blk.device, n_dev);
            block_rows(part_of(p), k, &blk.r0, &blk.r1);
            SMH_TRY(use(blk));
            const size_t rows = blk.r1 - blk.r0;
            const uint32_t base = offset_rows[blk.r0];
            if (offset_rows[blk.r1] < base) return fail(SMH_ERR_INVALID, "offset_rows is not monotone");
            const size_t nnz = offset_rows[blk.r1] - base;
            off.resize(rows + 1);
            for (size_t i = 0; i <= rows; ++i) off[i] = offset_rows[blk.r0 + i] - base;  // local offsets, global columns
            SMH_TRY(smh_crs_create(dtype, rows, n_cols, nnz, off.data(), columns ? columns + base : nullptr,
                                   values ? (const char *)values + (size_t)base * vs : nullptr, validate, &blk.m));
            SMH_TRY(own_interval(blk, n_cols, &p->needs[k], &p->lo[k], &p->hi[k]));
        }
        return finish_par(p);
    }, out);
}

int smh_par_adopt(size_t n_blocks, smh_crs *const *blocks, size_t n_rows, smh_par **out) {
    return smh_par_adopt_split(n_blocks, blocks, n_rows, nullptr, out);
}

int smh_par_adopt_split(size_t n_blocks, smh_crs *const *blocks, size_t n_rows, const size_t *split_rows, smh_par **out) {
    if (!out || !blocks) return fail(SMH_ERR_INVALID, "NULL argument");
    if (split_rows && n_blocks) SMH_TRY(split_ok(n_blocks, n_rows, split_rows));
    // (block 0 gives the handle its dtype and its columns; the NULL blocks are named by the fill step, after make_par's own checks)
    const smh_crs *first = n_blocks ? blocks[0] : nullptr;
    return make_par(first ? first->dtype : SMH_F32, n_blocks, n_blocks, n_rows, first ? first->n_cols : 0, nullptr, [&](smh_par *p) -> int {
        for (size_t k = 0; k < n_blocks; ++k)
            if (!blocks[k]) return fail(SMH_ERR_INVALID, "block %zu is NULL", k);
        if (split_rows) p->split.assign(split_rows, split_rows + n_blocks + 1);
        for (size_t k = 0; k < n_blocks; ++k) {
            ParBlock &blk = p->b[k];
            blk.index = k;
            blk.m = blocks[k];
            blk.owns_m = false;
            blk.device = blk.m->device;
            block_rows(part_of(p), k, &blk.r0, &blk.r1);
            if (blk.m->dtype != p->dtype || blk.m->n_cols != p->n_cols)
                return fail(SMH_ERR_INVALID, "block %zu: dtype / n_cols differ from block 0", k);
            if (blk.m->n_rows != blk.r1 - blk.r0)
                return fail(SMH_ERR_DIM_MISMATCH, "block %zu has %zu rows, the partition of %zu rows into %zu blocks gives it %zu", k,
                            blk.m->n_rows, n_rows, n_blocks, blk.r1 - blk.r0);
            SMH_TRY(use(blk));
            SMH_TRY(own_interval(blk, p->n_cols, &p->needs[k], &p->lo[k], &p->hi[k]));
        }
        return finish_par(p);
    }, out);
}

int smh_par_create_rank(smh_comm *comm, size_t n_rows, smh_crs *block, smh_par **out) {
    return smh_par_create_rank_split(comm, n_rows, block, (size_t)-1, out);
}

// row_begin == (size_t)-1: the reference's partition (this rank's block must hold rows [rank R, (rank + 1) R), the last rank also
// the remainder); else this rank's block holds the rows [row_begin, row_begin + its row count) and the ranks' ranges, all-gathered
// here, must tile [0, n_rows) in rank order (every rank passes a row_begin, or none does)
int smh_par_create_rank_split(smh_comm *comm, size_t n_rows, smh_crs *block, size_t row_begin, smh_par **out) {
    if (!out || !comm || !block) return fail(SMH_ERR_INVALID, "NULL argument");
    const bool own_split = row_begin != (size_t)-1;
    const size_t n_blocks = (size_t)comm->n_ranks, k = (size_t)comm->rank;
    return make_par(block->dtype, n_blocks, 1, n_rows, block->n_cols, comm, [&](smh_par *p) -> int {
        if (block->device != comm->device) return fail(SMH_ERR_INVALID, "the block lives on device %d, the communicator rank on device %d", block->device, comm->device);
        ParBlock &blk = p->b[0];
        blk.index = k;
        blk.m = block;
        blk.owns_m = false;
        blk.device = block->device;
        if (own_split) { blk.r0 = row_begin; blk.r1 = row_begin + block->n_rows; }
        else block_rows(part_of(p), k, &blk.r0, &blk.r1);
        // Everything a rank can check ALONE happens before the gather, but a rank that fails it must not return while its peers
        // block inside the collective: it publishes the failure with its table row, every rank reads every row and all of them fail
        // (or succeed) together, with the same verdict.
        auto local = [&]() -> int {
            SMH_TRY(use(blk));
            SMH_TRY(finish_par(p));  // (streams and events first: independent of what the checks say)
            if (block->n_rows != blk.r1 - blk.r0 || blk.r1 > n_rows)
                return fail(SMH_ERR_DIM_MISMATCH, "rank %zu holds %zu rows, the partition of %zu rows into %zu blocks gives it %zu", k, block->n_rows,
                            n_rows, n_blocks, blk.r1 - blk.r0);
            return own_interval(blk, p->n_cols, &p->needs[k], &p->lo[k], &p->hi[k]);
        };
        const int lrc = local();
        const std::string lmsg = lrc == SMH_OK ? std::string() : std::string(smh_last_error());
        hipStream_t gs = blk.q.s.get() ? blk.q.s.get() : comm->s.get();  // (the communicator's own stream when this block's could not be made)
        // the ranks publish their column intervals and row ranges (the exchange plan is global): kPlanWords u32 per rank, all-gathered
        // in place in the communicator's scratch -- it has had room for the table since smh_comm_create, so nothing between the local
        // checks and the collective allocates
        constexpr size_t W = kPlanWords;
        std::vector<uint32_t> table(W * n_blocks, 0);
        table[W * k] = p->needs[k]; table[W * k + 1] = p->lo[k]; table[W * k + 2] = p->hi[k];
        table[W * k + 3] = (uint32_t)blk.r0; table[W * k + 4] = (uint32_t)((uint64_t)blk.r0 >> 32); table[W * k + 5] = own_split;
        table[W * k + 6] = (uint32_t)block->n_rows; table[W * k + 7] = (uint32_t)((uint64_t)block->n_rows >> 32); table[W * k + 8] = (uint32_t)lrc;
        uint32_t *d_table = reinterpret_cast<uint32_t *>(comm->d_scratch.get());
        SMH_HIP(hipMemcpyAsync(d_table, table.data(), W * n_blocks * sizeof(uint32_t), hipMemcpyHostToDevice, gs));
        SMH_NCCL(ncclAllGather(d_table + W * k, d_table, W, ncclUint32, comm->comm, gs));
        SMH_HIP(hipMemcpyAsync(table.data(), d_table, W * n_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, gs));
        SMH_HIP(hipStreamSynchronize(gs));
        // from here on every rank holds the same table and runs the same checks in the same order
        if (lrc != SMH_OK) return fail(lrc, "%s", lmsg.c_str());
        for (size_t q = 0; q < n_blocks; ++q)
            if (table[W * q + 8] != 0) return fail((int)table[W * q + 8], "rank %zu failed its local checks of the partition (status %u); no rank keeps a handle", q, table[W * q + 8]);
        for (size_t q = 0; q < n_blocks; ++q) { p->needs[q] = (uint8_t)table[W * q]; p->lo[q] = table[W * q + 1]; p->hi[q] = table[W * q + 2]; }
        size_t first_with = n_blocks, first_without = n_blocks;
        for (size_t q = n_blocks; q-- > 0;) (table[W * q + 5] ? first_with : first_without) = q;
        if (first_with < n_blocks && first_without < n_blocks)
            return fail(SMH_ERR_INVALID, "rank %zu passes a row_begin, rank %zu does not (all or none)", first_with, first_without);
        if (own_split) {
            p->split.assign(n_blocks + 1, n_rows);
            for (size_t q = 0; q < n_blocks; ++q) p->split[q] = (size_t)((uint64_t)table[W * q + 3] | (uint64_t)table[W * q + 4] << 32);
            // the ranges must tile [0, n_rows) in rank order: no gap, no overlap -- the WHOLE table, identically on every rank
            for (size_t q = 0; q < n_blocks; ++q) {
                const size_t rows_q = (size_t)((uint64_t)table[W * q + 6] | (uint64_t)table[W * q + 7] << 32);
                if (p->split[q] + rows_q != p->split[q + 1])
                    return fail(SMH_ERR_INVALID, "rank %zu: its rows [%zu, %zu) end at %zu, %s begins at %zu (the blocks must tile the rows in rank order)", q,
                                p->split[q], p->split[q] + rows_q, p->split[q] + rows_q, q + 1 < n_blocks ? "the next rank" : "the end of the matrix", p->split[q + 1]);
            }
            SMH_TRY(split_ok(n_blocks, n_rows, p->split.data()));
        }
        return SMH_OK;
    }, out);
}

int smh_par_destroy(smh_par *p) {
    if (!p) return SMH_OK;
    p->pool.stop();
    DeviceGuard g;
    for (ParBlock &blk : p->b) {
        (void)hipSetDevice(blk.device);
        if (blk.q.s.get()) (void)hipStreamSynchronize(blk.q.s.get());
    }
    vec_destroy(p->cg_p); vec_destroy(p->io_b); vec_destroy(p->io_x);
    for (ParBlock &blk : p->b) {
        (void)hipSetDevice(blk.device);
        if (blk.comm) (void)ncclCommDestroy(blk.comm);
        if (blk.q.sx.get()) (void)hipStreamSynchronize(blk.q.sx.get());
        blk.q.sx = Stream();
        blk.q.s = Stream();
        blk.q = BlockQueues();  // the events
        if (blk.owns_m) (void)smh_crs_destroy(blk.m);
        blk.io = HostStaging();
        blk.cg = CgWork();
    }
    delete p;  // (the pinned buffers)
    (void)hipGetLastError();
    return SMH_OK;
}

size_t smh_par_n_blocks(const smh_par *p) { return p ? p->n_blocks : 0; }
size_t smh_par_n_local_blocks(const smh_par *p) { return p ? p->b.size() : 0; }
size_t smh_par_n_rows(const smh_par *p) { return p ? p->n_rows : 0; }
size_t smh_par_n_cols(const smh_par *p) { return p ? p->n_cols : 0; }
size_t smh_par_rows_per_block(const smh_par *p) { return p ? p->rows_per_block : 0; }

size_t smh_par_nnz(const smh_par *p) {  // sparsemat_par.rs:117-123
    size_t n = 0;
    if (p) for (const ParBlock &blk : p->b) n += smh_crs_nnz(blk.m);
    return n;
}

int smh_par_block(const smh_par *p, size_t block, smh_crs **crs_out, size_t *row_begin, size_t *row_end, int *device) {
    if (!p || block >= p->b.size()) return fail(SMH_ERR_INVALID, "no such block");
    const ParBlock &blk = p->b[block];
    if (crs_out) *crs_out = blk.m;
    if (row_begin) *row_begin = blk.r0;
    if (row_end) *row_end = blk.r1;
    if (device) *device = blk.device;
    return SMH_OK;
}

int smh_par_block_stream(const smh_par *p, size_t block, void **stream_out) {
    if (!p || !stream_out || block >= p->b.size()) return fail(SMH_ERR_INVALID, "no such block");
    *stream_out = p->b[block].q.s.get();
    return SMH_OK;
}

int smh_par_get_block_and_row_id(const smh_par *p, size_t row, size_t *block_out, size_t *row_out) {
    if (!p || !block_out || !row_out) return fail(SMH_ERR_INVALID, "NULL argument");
    block_of_row(part_of(p), row, block_out, row_out);
    return SMH_OK;
}

int smh_par_split(const smh_par *p, size_t *rows_out) {
    if (!p || !rows_out) return fail(SMH_ERR_INVALID, "NULL argument");
    const Part pt = part_of(p);
    for (size_t k = 0; k < p->n_blocks; ++k) block_rows(pt, k, &rows_out[k], &rows_out[k + 1]);
    return SMH_OK;
}

int smh_par_scale(smh_par *p, double a) {  // sparsemat_par.rs:135-139
    if (!p) return fail(SMH_ERR_INVALID, "NULL handle");
    DeviceGuard g;
    for (ParBlock &blk : p->b) {
        SMH_TRY(use(blk));
        SMH_HIP(hipStreamSynchronize(blk.q.s.get()));
        SMH_TRY(smh_crs_scale(blk.m, a));
    }
    return SMH_OK;
}

int smh_par_set_backend(smh_par *p, int backend) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL handle");
    if (p->rank_comm) {
        if (backend == SMH_PAR_BACKEND_PEER) return fail(SMH_ERR_INVALID, "one process per GPU: the exchange is RCCL");
        return SMH_OK;
    }
    const bool distinct = distinct_devices(p);
    if (backend == SMH_PAR_BACKEND_AUTO) backend = distinct && p->b.size() > 1 ? SMH_PAR_BACKEND_RCCL : SMH_PAR_BACKEND_PEER;
    if (backend != SMH_PAR_BACKEND_PEER && backend != SMH_PAR_BACKEND_RCCL) return fail(SMH_ERR_INVALID, "unknown backend %d", backend);
    if (backend == SMH_PAR_BACKEND_RCCL && !distinct && p->b.size() > 1)
        return fail(SMH_ERR_INVALID, "RCCL backend: several blocks share a device (one device per block needed)");
    DeviceGuard g;
    SMH_TRY(sync_all(p));
    p->backend = backend;
    return SMH_OK;
}

int smh_par_backend(const smh_par *p) { return p ? p->backend : SMH_PAR_BACKEND_AUTO; }

int smh_par_set_threads(smh_par *p, int mode) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL handle");
    if (mode < -1 || mode > 1) return fail(SMH_ERR_INVALID, "mode must be -1 (automatic), 0 (one issuing thread) or 1 (a thread per local block)");
    DeviceGuard g;
    SMH_TRY(sync_all(p));
    p->use_threads = mode;
    if (!threads_wanted(p)) p->pool.stop();
    return SMH_OK;
}

int smh_par_synchronize(smh_par *p) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL handle");
    DeviceGuard g;
    return sync_all(p);
}

int smh_par_exchange_mode(const smh_par *p, int mode, int *resolved_out, size_t *max_recv_out) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL handle");
    int m = SMH_EXCHANGE_NONE;
    SMH_TRY(resolve_mode(p, mode, &m));
    if (resolved_out) *resolved_out = m;
    if (max_recv_out) plan_summary(part_of(p), nullptr, max_recv_out);
    return SMH_OK;
}

int smh_par_plan(size_t n_blocks, size_t n_rows, const uint8_t *needs, const uint32_t *lo, const uint32_t *hi, size_t block,
                 size_t *recv_begin, size_t *recv_end, size_t *send_begin, size_t *send_end, int *auto_mode_out, size_t *max_recv_out) {
    return smh_par_plan_split(n_blocks, n_rows, nullptr, needs, lo, hi, block, recv_begin, recv_end, send_begin, send_end, auto_mode_out, max_recv_out);
}

int smh_par_plan_split(size_t n_blocks, size_t n_rows, const size_t *split_rows, const uint8_t *needs, const uint32_t *lo, const uint32_t *hi,
                       size_t block, size_t *recv_begin, size_t *recv_end, size_t *send_begin, size_t *send_end, int *auto_mode_out,
                       size_t *max_recv_out) {
    if (n_blocks == 0 || (!split_rows && n_rows / n_blocks == 0)) return fail(SMH_ERR_INVALID, "rows per block would be 0 (sparsemat_par.rs:21,32)");
    if (!needs || !lo || !hi || block >= n_blocks) return fail(SMH_ERR_INVALID, "bad plan arguments");
    if (split_rows) SMH_TRY(split_ok(n_blocks, n_rows, split_rows));
    const Part pt{n_blocks, n_rows, split_rows, needs, lo, hi};
    for (size_t q = 0; q < n_blocks; ++q) {
        size_t a, e;
        recv_range(pt, block, q, &a, &e);
        if (recv_begin) recv_begin[q] = a;
        if (recv_end) recv_end[q] = e;
        recv_range(pt, q, block, &a, &e);
        if (send_begin) send_begin[q] = a;
        if (send_end) send_end[q] = e;
    }
    plan_summary(pt, auto_mode_out, max_recv_out);
    return SMH_OK;
}

// ---- distributed vectors -----------------------------------------------------------------------------------------------
int smh_par_vec_create(smh_par *p, size_t n, smh_par_vec **out) {
    if (!p || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    DeviceGuard g;
    return vec_create(p, n, out);
}

int smh_par_vec_destroy(smh_par_vec *v) {
    DeviceGuard g;
    vec_destroy(v);
    return SMH_OK;
}

size_t smh_par_vec_dim(const smh_par_vec *v) { return v ? v->n : 0; }

int smh_par_vec_upload(smh_par_vec *v, const void *host) {
    if (!v || (v->n && !host)) return fail(SMH_ERR_INVALID, "NULL argument");
    smh_par *p = v->p;
    const size_t vs = dtype_size(p->dtype);
    return issue(p, [&]() -> int {
        for (size_t k = 0; k < p->b.size(); ++k) {
            SMH_TRY(use(p->b[k]));
            if (v->n) SMH_HIP(hipMemcpyAsync(v->d[k].get(), host, v->n * vs, hipMemcpyHostToDevice, p->b[k].q.s.get()));
        }
        return sync_all(p);  // the host buffer is borrowed for the call only
    });
}

int smh_par_vec_download(const smh_par_vec *v, void *host) {
    if (!v || !host) return fail(SMH_ERR_INVALID, "NULL argument");
    smh_par *p = v->p;
    if (v->n != p->n_rows) return fail(SMH_ERR_DIM_MISMATCH, "the vector has %zu entries, the partition owns %zu rows", v->n, p->n_rows);
    const size_t vs = dtype_size(p->dtype);
    return issue(p, [&]() -> int {
        for (size_t k = 0; k < p->b.size(); ++k) {
            const ParBlock &blk = p->b[k];
            SMH_TRY(use(blk));
            if (blk.r1 > blk.r0)
                SMH_HIP(hipMemcpyAsync((char *)host + blk.r0 * vs, (const char *)v->d[k].get() + blk.r0 * vs, (blk.r1 - blk.r0) * vs, hipMemcpyDeviceToHost, blk.q.s.get()));
        }
        return sync_all(p);
    });
}

int smh_par_vec_download_block(const smh_par_vec *v, size_t local_block, void *host) {
    if (!v || !host || local_block >= v->d.size()) return fail(SMH_ERR_INVALID, "bad argument");
    DeviceGuard g;
    const ParBlock &blk = v->p->b[local_block];
    SMH_TRY(use(blk));
    if (v->n) SMH_HIP(hipMemcpyAsync(host, v->d[local_block].get(), v->n * dtype_size(v->p->dtype), hipMemcpyDeviceToHost, blk.q.s.get()));
    SMH_HIP(hipStreamSynchronize(blk.q.s.get()));
    return SMH_OK;
}

int smh_par_vec_ptr(const smh_par_vec *v, size_t local_block, void **dev_ptr_out) {
    if (!v || !dev_ptr_out || local_block >= v->d.size()) return fail(SMH_ERR_INVALID, "bad argument");
    *dev_ptr_out = v->d[local_block].get();
    return SMH_OK;
}

}  // extern "C"
