// par_cg.hip -- ConjugateGradient::solve (linearsolver.rs:27-61) on the partitioned matrix: x, r, p, Ap distributed by rows; per
// iteration one WINDOW exchange of p, the local SpMV, and two cross-block folds whose operands stay on the devices: each block reduces
// its rows to one value, the values meet (the seam of par.hpp: slots in pinned host memory every device maps, ordered by events, or a
// 1-element all-gather) and every block folds the same n_blocks values with the same fixed tree -> identical alpha / beta / stop
// decision on all blocks, no host round trip, bitwise reproducible.  The host polls the stop flag every check_every iterations; the
// gated kernels of later iterations are no-ops (cg.hip), so x is exactly the x of the iteration that converged.
#include "par.hpp"

#include <chrono>
#include <cstdlib>
#include <cstring>

using namespace smh;
using namespace smh::par;

namespace smh {
// cg.hip
int cg_fold(int dtype, const void *partials, uint32_t count, void *out, hipStream_t s);
int cg_par_init(int dtype, void *sc, double tol, size_t iter_max, hipStream_t s);
int cg_par_set_rr(int dtype, void *sc, const void *vals, uint32_t nb, hipStream_t s);
int cg_par_update(int dtype, const void *sc_in, void *sc_out, const void *pap_vals, uint32_t nb, void *r, const void *ap, size_t n, void *partials,
                  uint32_t *count_out, hipStream_t s);
int cg_par_p(int dtype, const void *sc_in, void *sc_out, const void *rr_vals, uint32_t nb, void *p, const void *r, void *x, size_t n, hipStream_t s);

namespace par {

int ensure_cg_state(smh_par *p) {
    const size_t vs = dtype_size(p->dtype);
    for (ParBlock &blk : p->b) {
        if (blk.cg.built) continue;
        SMH_TRY(use(blk));
        const size_t n_loc = blk.r1 - blk.r0;
        CgWork w;  // (an early return frees what it holds; the block is touched at the last line only)
        SMH_TRY(w.r.alloc((n_loc ? n_loc : 1) * vs));
        SMH_TRY(w.ap.alloc((n_loc ? n_loc : 1) * vs));
        SMH_TRY(w.partials.alloc(((size_t)kReducePartials + 8) * vs));
        w.dotp_cap = (n_loc + 255) / 256 + 8;
        SMH_TRY(w.dotp.alloc(w.dotp_cap * vs));
        SMH_TRY(w.redv.alloc(2 * p->n_blocks * vs));
        SMH_HIP(hipMemset(w.redv.get(), 0, 2 * p->n_blocks * vs));
        SMH_TRY(w.sc.alloc(cg_scalars_bytes(p->dtype)));
        SMH_TRY(w.sc2.alloc(cg_scalars_bytes(p->dtype)));
        w.built = true;
        blk.cg = std::move(w);
    }
    if (!p->h_red.get()) {
        SMH_TRY(p->h_red.alloc(2 * p->n_blocks * sizeof(double), hipHostMallocPortable | hipHostMallocMapped));
        memset(p->h_red.get(), 0, 2 * p->n_blocks * sizeof(double));
    }
    if (!p->h_sc.get()) SMH_TRY(p->h_sc.alloc(cg_scalars_bytes(p->dtype), hipHostMallocDefault));
    return SMH_OK;
}

}  // namespace par
}  // namespace smh

extern "C" {

int smh_par_cg_solve_vec(smh_par *p, const smh_par_vec *b, smh_par_vec *x, double tol, size_t iter_max, int variant,
                         size_t check_every, size_t *iters_out, double *rr_out) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(check_vec(p, b, "b"));
    SMH_TRY(check_vec(p, x, "x"));
    if (b == x) return fail(SMH_ERR_INVALID, "b and x must be different vectors");
    if (p->n_rows != p->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");                        // :30-32
    if (p->n_rows != b->n || p->n_rows != x->n) return fail(SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch");  // :33-36
    if (check_every == 0) check_every = 8;
    const size_t vs = dtype_size(p->dtype), n = p->n_rows;
    const int dt = p->dtype;
    const uint32_t nb = (uint32_t)p->n_blocks;
    size_t iters = 0;
    double rr = 0.0;
    SMH_TRY(issue(p, [&]() -> int {
        SMH_TRY(ensure_cg_state(p));
        if (!p->cg_p) SMH_TRY(vec_create(p, n, &p->cg_p));
        smh_par_vec *pv = p->cg_p;
        int mode = SMH_EXCHANGE_NONE;
        SMH_TRY(resolve_mode(p, SMH_EXCHANGE_AUTO, &mode));
        // r = b - A x (:38); p = r.clone() (:39); rr = r.r (:40)
        SMH_TRY(exchange(p, x, mode));  // x on every block's column interval
        for (size_t k = 0; k < p->b.size(); ++k) {
            ParBlock &blk = p->b[k];
            SMH_TRY(use(blk));
            const size_t n_loc = blk.r1 - blk.r0;
            SMH_TRY(smh_crs_spmv_dev(blk.m, x->d[k].get(), n, blk.cg.r.get(), variant, blk.q.s.get()));
            SMH_TRY(launch_ew(dt, Ew::RSubInto, blk.cg.r.get(), (const char *)b->d[k].get() + blk.r0 * vs, n_loc, 0.0, nullptr, blk.q.s.get()));
            SMH_HIP(hipMemcpyAsync((char *)pv->d[k].get() + blk.r0 * vs, blk.cg.r.get(), n_loc * vs, hipMemcpyDeviceToDevice, blk.q.s.get()));
            SMH_TRY(cg_par_init(dt, blk.cg.sc.get(), tol, iter_max, blk.q.s.get()));
            SMH_TRY(launch_dot(dt, blk.cg.r.get(), blk.cg.r.get(), n_loc, blk.cg.partials.get(), fold_mine(p, blk, 1), blk.q.s.get()));
        }
        SMH_TRY(combine(p, 1));
        for (ParBlock &blk : p->b) {
            SMH_TRY(use(blk));
            SMH_TRY(cg_par_set_rr(dt, blk.cg.sc.get(), fold_values(p, blk, 1), nb, blk.q.s.get()));
        }
        // the entries of p a block references and another owns -- beside the product of the interior rows, which need none of them,
        // when the exchange is a window (the rows that do wait for it at the join)
        const bool side = overlapped(p, mode);
        // the product of block k's rows [part 0: its interior, on the main stream | part 1: the rest -- on the SIDE stream, behind the
        // exchange they wait for and beside the interior rows -- or, unsplit, nothing | part 2, after the join: unsplit, all rows; the
        // block's p.Ap]
        auto products = [&](size_t k, int part) -> int {
            ParBlock &blk = p->b[k];
            SMH_TRY(use(blk));
            const size_t n_loc = blk.r1 - blk.r0;
            size_t ia = 0, ie = 0;
            if (side) SMH_TRY(interior_for(blk, variant, &ia, &ie));
            const bool split = ie > ia;
            if (part == 0 && !split) return SMH_OK;
            // :43 and :45 -- with the CSR-stream kernel p.Ap rides the product's epilogue (one partial per tile, lhs = this
            // block's slice of p) as in the single-matrix solver: no second pass over p and Ap
            const size_t n_dot = spmv_fused_dot_partials(blk.m, n, variant, true);
            const bool fused = n_dot && n_dot <= blk.cg.dotp_cap;
            void *dotp = fused ? blk.cg.dotp.get() : nullptr;
            const void *lhs = fused ? (const char *)pv->d[k].get() + blk.r0 * vs : nullptr;
            if (part == 0) return spmv_enqueue_rows(blk.m, pv->d[k].get(), n, blk.cg.ap.get(), variant, blk.q.s.get(), ia, ie, dotp, lhs);
            if (part == 1 && split) {
                if (!dotp) {
                    SMH_TRY(spmv_enqueue_rows_short(blk.m, pv->d[k].get(), n, blk.cg.ap.get(), variant, blk.q.sx.get(), 0, ia));
                    return spmv_enqueue_rows_short(blk.m, pv->d[k].get(), n, blk.cg.ap.get(), variant, blk.q.sx.get(), ie, n_loc);
                }
                SMH_TRY(spmv_enqueue_rows(blk.m, pv->d[k].get(), n, blk.cg.ap.get(), variant, blk.q.sx.get(), 0, ia, dotp, lhs));
                return spmv_enqueue_rows(blk.m, pv->d[k].get(), n, blk.cg.ap.get(), variant, blk.q.sx.get(), ie, n_loc, dotp, lhs);
            }
            if (part == 1) return SMH_OK;  // (unsplit: everything in part 2, after the exchange has been joined)
            if (!split) {
                if (fused) SMH_TRY(spmv_enqueue(blk.m, pv->d[k].get(), n, blk.cg.ap.get(), variant, blk.q.s.get(), blk.cg.dotp.get(), lhs));
                else SMH_TRY(smh_crs_spmv_dev(blk.m, pv->d[k].get(), n, blk.cg.ap.get(), variant, blk.q.s.get()));
            }
            if (fused) return launch_fold2(dt, blk.cg.dotp.get(), n_dot, blk.cg.partials.get(), fold_mine(p, blk, 0), blk.q.s.get());
            return launch_dot(dt, (const char *)pv->d[k].get() + blk.r0 * vs, blk.cg.ap.get(), n_loc, blk.cg.partials.get(), fold_mine(p, blk, 0), blk.q.s.get());
        };
        auto update_xr = [&](size_t k) -> int {  // alpha, then x / r and this block's share of r.r
            ParBlock &blk = p->b[k];
            SMH_TRY(use(blk));
            uint32_t cnt = 0;
            SMH_TRY(cg_par_update(dt, blk.cg.sc.get(), blk.cg.sc2.get(), fold_values(p, blk, 0), nb, blk.cg.r.get(), blk.cg.ap.get(), blk.r1 - blk.r0, blk.cg.partials.get(), &cnt, blk.q.s.get()));  // :45, :49-51
            return cg_fold(dt, blk.cg.partials.get(), cnt, fold_mine(p, blk, 1), blk.q.s.get());
        };
        auto update_p = [&](size_t k) -> int {  // beta (and the stop test before it), then p
            ParBlock &blk = p->b[k];
            SMH_TRY(use(blk));
            return cg_par_p(dt, blk.cg.sc2.get(), blk.cg.sc.get(), fold_values(p, blk, 1), nb, (char *)pv->d[k].get() + blk.r0 * vs, blk.cg.r.get(), (char *)x->d[k].get() + blk.r0 * vs,
                            blk.r1 - blk.r0, blk.q.s.get());  // :52-56, :47, :58-59
        };
        // ---- one iteration (:41-60) as phases: within a phase every block's calls are issued by its own host thread (par_for);
        // between phases all of them have been issued -- what a wait on another block's event needs, and where the caller issues
        // what is one call for all blocks.  Streams, events, kernels and their order per block are those of the one-thread form,
        // whatever the number of threads and whichever backend stands behind the seam.
        auto iteration = [&]() -> int {
            if (mode != SMH_EXCHANGE_NONE) SMH_TRY(par_for(p, [&](size_t k) -> int {
                if (side) SMH_TRY(fork_one(p->b[k]));
                return xchg_begin(p, k, mode, side);
            }));
            SMH_TRY(xchg_all(p, pv, mode, side));
            SMH_TRY(par_for(p, [&](size_t k) -> int {
                SMH_TRY(xchg_pull(p, k, pv, mode, side));
                return side ? products(k, 0) : SMH_OK;
            }));
            SMH_TRY(par_for(p, [&](size_t k) -> int {
                if (side) SMH_TRY(products(k, 1));  // (behind this block's exchange on its side stream)
                SMH_TRY(xchg_end(p, k, mode, side));
                if (side) SMH_TRY(join_one(p->b[k]));
                SMH_TRY(products(k, 2));
                return fold_put(p, k, 0);
            }));
            SMH_TRY(fold_all(p, 0));
            SMH_TRY(par_for(p, [&](size_t k) -> int {
                SMH_TRY(fold_get(p, k, 0));
                SMH_TRY(update_xr(k));
                return fold_put(p, k, 1);
            }));
            SMH_TRY(fold_all(p, 1));
            return par_for(p, [&](size_t k) -> int {
                SMH_TRY(fold_get(p, k, 1));
                return update_p(k);
            });
        };
        size_t launched = 0;
        int converged = 0;
        auto poll = [&]() -> int {
            ParBlock &b0 = p->b[0];
            SMH_TRY(use(b0));
            SMH_HIP(hipMemcpyAsync(p->h_sc.get(), b0.cg.sc.get(), cg_scalars_bytes(dt), hipMemcpyDeviceToHost, b0.q.s.get()));
            // (block 0's stream alone: its scalars are every block's scalars -- all fold the same values -- and the other blocks'
            // streams keep their queues full across the poll; everything is drained once, when the solve returns)
            SMH_HIP(hipStreamSynchronize(b0.q.s.get()));
            uint64_t it64 = 0;
            cg_read_scalars(dt, p->h_sc.get(), &converged, &it64, &rr);
            iters = (size_t)it64;
            return SMH_OK;
        };
        while (launched < iter_max) {
            const size_t batch = iter_max - launched < check_every ? iter_max - launched : check_every;
            static const bool trace = getenv("SMH_PAR_TRACE") && atoi(getenv("SMH_PAR_TRACE")) != 0;  // development aid
            const auto t_a = std::chrono::steady_clock::now();
            for (size_t i = 0; i < batch; ++i) SMH_TRY(iteration());
            const auto t_b = std::chrono::steady_clock::now();
            launched += batch;
            SMH_TRY(poll());
            if (trace) {
                const auto t_c = std::chrono::steady_clock::now();
                fprintf(stderr, "[par cg] %zu iterations: issued in %.3f ms (%.3f per iteration), drained %.3f ms later\n", batch,
                        std::chrono::duration<double, std::milli>(t_b - t_a).count(), std::chrono::duration<double, std::milli>(t_b - t_a).count() / (double)batch,
                        std::chrono::duration<double, std::milli>(t_c - t_b).count());
            }
            if (converged) break;
        }
        if (iter_max == 0) SMH_TRY(poll());
        return sync_all(p);
    }));
    if (iters_out) *iters_out = iters;
    if (rr_out) *rr_out = rr;
    return SMH_OK;
}

int smh_par_cg_solve(smh_par *p, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len, double tol, size_t iter_max,
                     int variant, size_t *iters_out, double *rr_out) {
    if (!p) return fail(SMH_ERR_INVALID, "NULL handle");
    if (p->n_rows != p->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");                    // :30-32
    if (p->n_rows != b_len || p->n_rows != x_len) return fail(SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch");  // :33-36
    if (!b_host || !x_host_inout) return fail(SMH_ERR_INVALID, "NULL host vector");
    return issue(p, [&]() -> int {
        if (!p->io_b) SMH_TRY(vec_create(p, p->n_rows, &p->io_b));
        if (!p->io_x) SMH_TRY(vec_create(p, p->n_rows, &p->io_x));
        SMH_TRY(smh_par_vec_upload(p->io_b, b_host));
        SMH_TRY(smh_par_vec_upload(p->io_x, x_host_inout));
        SMH_TRY(smh_par_cg_solve_vec(p, p->io_b, p->io_x, tol, iter_max, variant, 0, iters_out, rr_out));
        return smh_par_vec_download(p->io_x, x_host_inout);
    });
}

}  // extern "C"
