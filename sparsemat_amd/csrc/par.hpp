// par.hpp -- what the units of the partitioned path share (private): the handles, the issuing of phases, the one way out of an
// entry point, and the SEAM between the steps and the two exchange backends.
//   par.hip       communicators, construction and destruction, accessors, distributed vectors
//   par_step.hip  the kernels, the backends behind the seam, interiors, the product step and the exchange
//   par_cg.hip    the CG's state and the solver
#pragma once

#include "internal.hpp"
#include "par_issue.hpp"
#include "par_plan.hpp"

#include <rccl/rccl.h>

#include <string>
#include <vector>

#define SMH_NCCL(call)                                                                                    \
    do {                                                                                                  \
        ncclResult_t r__ = (call);                                                                        \
        if (r__ != ncclSuccess)                                                                           \
            return ::smh::fail(SMH_ERR_COMM, "%s failed: %s (%s:%d)", #call, ncclGetErrorString(r__), __FILE__, __LINE__); \
    } while (0)

struct smh_comm {
    ncclComm_t comm = nullptr;
    int n_ranks = 1, rank = 0, device = 0;
    smh::Stream s;  // for the host-facing helpers (barrier, max)
    smh::DevArray<char> d_scratch;  // the helpers' operand, and the table smh_par_create_rank_split gathers: kPlanWords u32 per rank
};

namespace smh {
namespace par {

constexpr size_t kPlanWords = 9;  // per rank: needs, lo, hi, row_begin (low, high word), has its own split, row count (low, high word), local status

// What a block owns beside its matrix, in three members.  The two that are built on first use are filled in a local instance and
// move-assigned into the block when every array exists (`built`): a failed build leaves the block as it was, holding nothing.
struct BlockQueues {  // streams and events (finish_par)
    Stream s;
    Stream sx;          // the exchange's stream when it runs beside the interior rows' product
    Event fork, join;   // s -> sx (what the exchange needs is written), sx -> s (the exchange is done)
    Event slice;        // own slice of the vector being exchanged is written
    Event done;         // this block's pulls from its peers are complete
    Event red[2];       // its value of fold slot 0 / 1 is written
    Event all[2];       // (block 0) every block's value of the slot is written
};
struct CgWork {  // CG state (first solve; ensure_cg_state)
    bool built = false;
    DevArray<char> r, ap, partials;
    DevArray<char> dotp;     // the SpMV's p.Ap partials (one per 256-row tile), folded by launch_fold2 through partials
    size_t dotp_cap = 0;
    DevArray<char> sc, sc2;  // the scalars are double-buffered: the alpha / update launch reads sc and writes sc2, the beta / p launch back (cg.hip)
    DevArray<char> redv;     // RCCL backend: 2 x n_blocks values (fold slots)
};
struct HostStaging {  // staging of the host-vector API (smh_par_spmv)
    bool built = false;
    DevArray<char> x, y;
};

struct ParBlock {
    size_t index = 0;             // global block id
    int device = 0;
    smh_crs *m = nullptr;
    bool owns_m = true;
    size_t r0 = 0, r1 = 0;        // global rows [r0, r1)
    // INTERIOR rows [in0, in1) (local): no other block references them and they reference no other block's columns, so their
    // product needs nothing from the exchange and gives nothing to it (in1 <= in0: none)
    size_t in0 = 0, in1 = 0;
    ncclComm_t comm = nullptr;    // RCCL backend: this block's rank of the communicator
    BlockQueues q;
    CgWork cg;
    HostStaging io;
};

}  // namespace par
}  // namespace smh

struct smh_par {
    int dtype = SMH_F32;
    size_t n_rows = 0, n_cols = 0, rows_per_block = 0, n_blocks = 0;
    std::vector<smh::par::ParBlock> b;  // LOCAL blocks: all of them (one process), or this rank's (one process per GPU)
    smh_comm *rank_comm = nullptr;  // one process per GPU (borrowed)
    int backend = SMH_PAR_BACKEND_PEER;  // resolved
    bool comms_ready = false;
    bool overlap = true;            // window exchanges run beside the interior rows' product (smh_par_set_overlap; SMH_PAR_OVERLAP=0)
    // column intervals of ALL blocks: block q references [lo[q], hi[q]] when needs[q]
    std::vector<uint32_t> lo, hi;
    std::vector<uint8_t> needs;
    std::vector<size_t> split;      // empty: the reference's partition (R rows per block); else n_blocks + 1 row boundaries
    std::vector<uint8_t> peer_ok;   // [dst local * n_local + src local]: dst's device can read src's memory directly
    std::vector<uint8_t> pulled;    // the PEER exchange in flight: [q * n_local + src] = q read from src (its pull step to its end step)
    smh::PinnedBuf h_red;           // PEER backend: 2 x n_blocks fold slots in pinned host memory (all devices map it)
    smh::PinnedBuf h_sc;            // pinned copy of block 0's CG scalars
    smh_par_vec *cg_p = nullptr;    // the search direction of the solver (full-length per block)
    smh_par_vec *io_b = nullptr, *io_x = nullptr;  // staging of the host-vector solve
    smh::IssuePool pool;            // issuing threads (started by the first phase that wants them; blocks 1 .. n_local - 1)
    int use_threads = -1;           // -1 automatic (= off unless SMH_PAR_THREADS=1: threads_wanted() says why), 0 never, 1 always
};

struct smh_par_vec {
    smh_par *p = nullptr;
    size_t n = 0;
    std::vector<smh::DevArray<char>> d;  // per local block, n entries on its device
};

namespace smh {
namespace par {

using namespace smh::plan;

// ---- par.hip ---------------------------------------------------------------------------------------------------------------
int use(const ParBlock &blk);  // before every runtime call of a block: the thread is on the block's device
struct DeviceGuard {
    int prev = 0;
    DeviceGuard() { (void)hipGetDevice(&prev); }
    ~DeviceGuard() { (void)hipSetDevice(prev); }
};
int sync_all(smh_par *p);  // both streams of every block
bool threads_wanted(const smh_par *p);
inline Part part_of(const smh_par *p) { return Part{p->n_blocks, p->n_rows, p->split.empty() ? nullptr : p->split.data(), p->needs.data(), p->lo.data(), p->hi.data()}; }
int vec_create(smh_par *p, size_t n, smh_par_vec **out);
void vec_destroy(smh_par_vec *v);
int check_vec(const smh_par *p, const smh_par_vec *v, const char *what);

// fn(k) for every local block k -- concurrently, one thread per block, when the handle has its issuing threads; returns when all
// have returned (a HOST barrier: what fn issued is on the streams, not necessarily executed), with the first failure
template <class F> int par_for(smh_par *p, F &&fn) {
    const int rc = p->pool.run(p->b.size(), fn, threads_wanted(p));
    if (rc != SMH_OK && p->pool.message()) return fail(rc, "%s", p->pool.message());  // (a worker's text, or an exception's)
    return rc;
}

// THE WAY OUT of every entry point that issues onto the blocks' streams: the caller's device restored, and after a failure -- some
// blocks may have forked, launched or begun an exchange that others never joined -- both streams of every block drained before the
// status goes back with its text.  The handle is usable again at once.
template <class F> int issue(smh_par *p, F &&body) {
    DeviceGuard g;
    const int rc = body();
    if (rc != SMH_OK) return keep_error(rc, [&] { (void)sync_all(p); });
    return SMH_OK;
}

// ---- par_step.hip: the seam.  A step never asks which backend is active; it runs these parts in phases (P: par_for, C: caller) ----
// exchange of v (mode: resolved; NONE: every part does nothing), on the blocks' side streams when `side`:
//   P xchg_begin | C xchg_all | P xchg_pull | P xchg_end       PEER: mark / - / pull / guard       RCCL: - / the group(s) / - / -
int xchg_begin(smh_par *p, size_t k, int mode, bool side);
int xchg_all(smh_par *p, smh_par_vec *v, int mode, bool side);
int xchg_pull(smh_par *p, size_t k, smh_par_vec *v, int mode, bool side);
int xchg_end(smh_par *p, size_t k, int mode, bool side);
// fold slot 0 / 1, after block k wrote fold_mine (a lone block: every part does nothing):
//   P fold_put | C fold_all | P fold_get, then block k reads fold_values      PEER: mark / hub / wait      RCCL: - / all-gather / -
int fold_put(smh_par *p, size_t k, int slot);
int fold_all(smh_par *p, int slot);
int fold_get(smh_par *p, size_t k, int slot);
void *fold_values(const smh_par *p, const ParBlock &blk, int slot);  // all n_blocks values, as block blk reads them
void *fold_mine(const smh_par *p, const ParBlock &blk, int slot);    // where block blk's own value goes
// the parts as whole steps
int exchange(smh_par *p, smh_par_vec *v, int mode, bool side = false);  // mode as given by the caller; resolves and checks it
int combine(smh_par *p, int slot);

bool lone_block_skips(const smh_par *p);
int resolve_mode(const smh_par *p, int mode, int *out);
bool distinct_devices(const smh_par *p, size_t *i = nullptr, size_t *j = nullptr);
// side streams
int fork_one(ParBlock &blk);
int join_one(ParBlock &blk);
bool overlapped(const smh_par *p, int resolved_mode);
int interior_for(ParBlock &blk, int variant, size_t *a, size_t *e);
int find_interiors(smh_par *p);

// ---- par_cg.hip ----------------------------------------------------------------------------------------------------------------
int ensure_cg_state(smh_par *p);

}  // namespace par
}  // namespace smh
