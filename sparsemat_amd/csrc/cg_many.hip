// cg_many.hip -- K5m: ConjugateGradient::solve (reference linearsolver.rs:27-61) on k right-hand sides at once.
//
// k independent recurrences, one per column of the multi-vectors B and X, each exactly the one cg.hip restates -- its own alpha,
// beta, stop test and iteration count -- that share ONE sweep over the matrix per body (K1m, spmv_many.hip) and fused
// multi-vector update kernels.  Per body, all on the handle's stream and without a host synchronisation:
//
//   smh_crs_spmv_many_dev   AP = A P                       (ceil(ld / 4) sweeps)                                        :43
//   k_mvec_dot              per-column partials of p.Ap    (mvec_blas.hip)                                              :45
//   k_cgm_update            every workgroup folds the p.Ap partials of its row group's columns; alpha_c = rr_c / pAp_c,
//                           "active"; r_c -= round(Ap_c * alpha_c); per-column partials of r.r                          :45, :49-51
//   k_cgm_p                 folds the r.r partials; stop if sqrt(f64(rr_c)) < tol, else beta_c = rr_c / rr_prev_c;
//                           x_c += round(p_c * alpha_c) (:47), p_c = round(p_c * beta_c) + r_c where column c goes on  :51-59
//
// A column is ACTIVE while it has not converged and has entered fewer than iter_max bodies.  An inactive column's x, r and p are
// kept BY SELECTION (the value read is the value stored -- no multiplication by a zero alpha), so a column that stopped early
// keeps the bits of its stopping body, and a NaN recurrence (b_c = 0: 0 / 0) runs to iter_max beside its neighbours without
// touching them: no value of one column enters another column's arithmetic anywhere.  Padding columns (c >= k) are created
// converged; they stay +0 in X, R, P (never written with other bits) and in AP (K1m stores +0 there).
//
// Every reduction sums column c in the column tree of mvec_tree.hpp / mvec_blas.hip, whose order depends on n alone.
//
// The scalars: an array of ld + 1 CgScalars<T> blocks, [0] a summary for the batch driver (solve_in_batches polls it: `converged`
// = no column active, `iters` = bodies any column entered), [1 + c] column c's.  They are double-buffered like the single
// solver's: k_cgm_update reads `in` and writes `out`, k_cgm_p the other way round; within a launch the workgroup (group, 0)
// writes its group's columns and every other workgroup takes the same decisions from `in` and the same fold.  The summary is
// taken from `in` at the head of a body, so the host learns of the last column's stop with the first body AFTER it (a
// no-op): folding every column's r.r in one workgroup for it would cost O(k) folds per body.
#include "mvec_tree.hpp"
#include "solver_host.hpp"

namespace smh {

template <typename T>
__device__ __forceinline__ bool cgm_active(const CgScalars<T> &c) { return !c.converged && c.iters < c.iter_max; }

// [1 + c].rr = fold of column c's partials of the initial r.r (:40); padding columns are created converged
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_cgm_init(CgScalars<T> *__restrict__ sc, const T *__restrict__ partials, uint32_t nb, uint32_t k, uint32_t ld, double tol, uint64_t iter_max) {
    __shared__ T s_w[1][kBlock / kWave];
    __shared__ T s_sum[1];
    CgScalars<T> o;
    o.rr = o.rr_prev = o.pap = o.alpha = o.beta = T(0);
    o.converged = o.active = o.entered = o.pad_ = 0;
    o.iters = 0;
    o.iter_max = iter_max;
    o.tol = tol;
    if (blockIdx.x == 0 && threadIdx.x == 0) sc[0] = o;
    for (uint32_t c = blockIdx.x; c < ld; c += gridDim.x) {
        mv_fold_group<T, 1>(partials, nb, c, s_w, s_sum);
        if (threadIdx.x == 0) {
            o.rr = s_sum[0];
            o.converged = c >= k ? 1u : 0u;
            sc[1 + c] = o;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_cgm_update(const CgScalars<T> *__restrict__ in, CgScalars<T> *__restrict__ out, const T *__restrict__ pap_part, uint32_t nb,
             T *__restrict__ r, const T *__restrict__ ap, uint64_t n, uint32_t ngroups, uint32_t k, T *__restrict__ rr_part) {
    typedef typename MvGroup<T>::type V;
    constexpr int G = MvGroup<T>::N;
    __shared__ T s_w[G][kBlock / kWave];
    __shared__ T s_sum[G];
    if (blockIdx.x == 0 && blockIdx.y == 0) {  // the summary
        int mine = 0;
        for (uint32_t c = threadIdx.x; c < k; c += kBlock) mine |= cgm_active(in[1 + c]) ? 1 : 0;
        const int any = __syncthreads_or(mine);
        if (threadIdx.x == 0) {
            CgScalars<T> o = in[0];
            o.active = o.entered = any ? 1u : 0u;
            if (any) o.iters += 1;
            else o.converged = 1;
            out[0] = o;
        }
    }
    V *rv = reinterpret_cast<V *>(r);
    const V *apv = reinterpret_cast<const V *>(ap);
    const uint64_t stride = (uint64_t)gridDim.y * kBlock;
    for (uint32_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        mv_fold_group<T, G>(pap_part, nb, grp * G, s_w, s_sum);
        T alpha[G];
        bool act[G], any = false;
#pragma unroll
        for (int e = 0; e < G; ++e) {
            const CgScalars<T> &ci = in[1 + grp * G + e];
            act[e] = cgm_active(ci);
            alpha[e] = act[e] ? ci.rr / s_sum[e] : ci.alpha;  // :45 (no breakdown guard, like the reference)
            any = any || act[e];
        }
        if (blockIdx.y == 0 && threadIdx.x < G) {
            CgScalars<T> o = in[1 + grp * G + threadIdx.x];
            const bool a = cgm_active(o);
            const T pap = s_sum[threadIdx.x];
            o.active = o.entered = a ? 1u : 0u;
            if (a) {
                o.alpha = o.rr / pap;
                o.pap = pap;
                o.iters += 1;  // a loop body is entered (for _k in 0..iter_max, :41)
            }
            out[1 + grp * G + threadIdx.x] = o;
        }
        if (!any) continue;  // (uniform over the grid's workgroups of this group: `in` is the same for all of them)
        T acc[G];
#pragma unroll
        for (int e = 0; e < G; ++e) acc[e] = T(0);
        for (uint64_t i = (uint64_t)blockIdx.y * kBlock + threadIdx.x; i < n; i += stride) {
            V rr = __builtin_nontemporal_load(rv + i * ngroups + grp);
            const V aa = __builtin_nontemporal_load(apv + i * ngroups + grp);
#pragma unroll
            for (int e = 0; e < G; ++e) {
                const T t = mv_sub(rr[e], mv_mul(aa[e], alpha[e]));  // r -= mat_p * alpha        :49
                rr[e] = act[e] ? t : rr[e];
                acc[e] += rr[e] * rr[e];                              // r.norm_squared()          :51
            }
            __builtin_nontemporal_store(rr, rv + i * ngroups + grp);
        }
        mv_block_sums<T, G>(acc, s_w, s_sum);
        if (threadIdx.x < G) rr_part[(uint64_t)(grp * G + threadIdx.x) * gridDim.y + blockIdx.y] = s_sum[threadIdx.x];
    }
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_cgm_p(const CgScalars<T> *__restrict__ in, CgScalars<T> *__restrict__ out, const T *__restrict__ rr_part, uint32_t nb, T *__restrict__ p,
        const T *__restrict__ r, T *__restrict__ x, uint64_t n, uint32_t ngroups) {
    typedef typename MvGroup<T>::type V;
    constexpr int G = MvGroup<T>::N;
    __shared__ T s_w[G][kBlock / kWave];
    __shared__ T s_sum[G];
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) out[0] = in[0];
    V *pv = reinterpret_cast<V *>(p);
    V *xv = reinterpret_cast<V *>(x);
    const V *rv = reinterpret_cast<const V *>(r);
    const uint64_t stride = (uint64_t)gridDim.y * kBlock;
    for (uint32_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        bool any = false;
#pragma unroll
        for (int e = 0; e < G; ++e) any = any || in[1 + grp * G + e].active != 0;
        if (!any) {  // no column of the group entered this body (uniform, as above)
            if (blockIdx.y == 0 && threadIdx.x < G) out[1 + grp * G + threadIdx.x] = in[1 + grp * G + threadIdx.x];
            continue;
        }
        mv_fold_group<T, G>(rr_part, nb, grp * G, s_w, s_sum);
        T alpha[G], beta[G];
        bool ent[G], reb[G], any_reb = false;
#pragma unroll
        for (int e = 0; e < G; ++e) {
            const CgScalars<T> &ci = in[1 + grp * G + e];
            const bool was = ci.active != 0;
            const T rr = s_sum[e];
            const bool conv = was && sqrt((double)rr) < ci.tol;  // :52-54, BEFORE the beta update
            ent[e] = ci.entered != 0;
            reb[e] = was && !conv;
            alpha[e] = ci.alpha;
            beta[e] = reb[e] ? rr / ci.rr : ci.beta;             // :56
            any_reb = any_reb || reb[e];
        }
        if (blockIdx.y == 0 && threadIdx.x < G) {
            CgScalars<T> o = in[1 + grp * G + threadIdx.x];
            if (o.active) {
                const T rr = s_sum[threadIdx.x];
                if (sqrt((double)rr) < o.tol) { o.converged = 1; o.active = 0; }
                else o.beta = rr / o.rr;
                o.rr_prev = o.rr;
                o.rr = rr;
            }
            out[1 + grp * G + threadIdx.x] = o;
        }
        if (any_reb) {
            for (uint64_t i = (uint64_t)blockIdx.y * kBlock + threadIdx.x; i < n; i += stride) {
                V pp = __builtin_nontemporal_load(pv + i * ngroups + grp), xx = __builtin_nontemporal_load(xv + i * ngroups + grp);
                const V rr = __builtin_nontemporal_load(rv + i * ngroups + grp);
#pragma unroll
                for (int e = 0; e < G; ++e) {
                    const T xn = mv_add(xx[e], mv_mul(pp[e], alpha[e]));  // *x += p.clone() * alpha        :47
                    const T pn = mv_add(mv_mul(pp[e], beta[e]), rr[e]);   // p.scale(beta); p.add(&r)       :58-59
                    xx[e] = ent[e] ? xn : xx[e];
                    pp[e] = reb[e] ? pn : pp[e];
                }
                __builtin_nontemporal_store(xx, xv + i * ngroups + grp);
                __builtin_nontemporal_store(pp, pv + i * ngroups + grp);
            }
        } else {  // every entered column of the group stopped in this body: x alone
            for (uint64_t i = (uint64_t)blockIdx.y * kBlock + threadIdx.x; i < n; i += stride) {
                V xx = __builtin_nontemporal_load(xv + i * ngroups + grp);
                const V pp = __builtin_nontemporal_load(pv + i * ngroups + grp);
#pragma unroll
                for (int e = 0; e < G; ++e) {
                    const T xn = mv_add(xx[e], mv_mul(pp[e], alpha[e]));
                    xx[e] = ent[e] ? xn : xx[e];
                }
                __builtin_nontemporal_store(xx, xv + i * ngroups + grp);
            }
        }
    }
}

template <typename T>
static int cg_solve_many_t(smh_crs *m, const smh_mvec *b, smh_mvec *x, double tol, size_t iter_max, size_t check_every, size_t *iters_out,
                           double *rr_out) {
    constexpr int G = MvGroup<T>::N;
    const size_t n = m->n_rows, k = b->k, ld = b->ld, ngroups = ld / G;
    hipStream_t s = m->stream;
    const unsigned nb = mv_tree_blocks(n);
    // the p sweep carries no reduction: its grid cannot change a bit (two workgroups per CU and row group at most, as cg.hip's)
    const unsigned pb = grid_for(n, 512);
    const unsigned gx = (unsigned)(ngroups < 1024 ? ngroups : 1024);
    DevArray<T> r, p, ap, pap_part, rr_part;
    DevArray<CgScalars<T>> sc, sc2;
    SolveRun run(s);  // (the workspaces here are exact-size DevArrays, not run.ws; run.iters / run.rr are the summary block's [0]: unused)
    std::vector<CgScalars<T>> h_all;
    try {
        h_all.resize(ld + 1);
    } catch (...) {
        return fail(SMH_ERR_OOM, "host allocation failed");
    }
    const int rc = run.run([&]() -> int {
        const size_t elems = n * ld ? n * ld : 4;
        SMH_TRY(r.alloc(elems));
        SMH_TRY(p.alloc(elems));
        SMH_TRY(ap.alloc(elems));
        SMH_TRY(pap_part.alloc(ld * (size_t)nb));
        SMH_TRY(rr_part.alloc(ld * (size_t)nb));
        SMH_TRY(sc.alloc(ld + 1));
        SMH_TRY(sc2.alloc(ld + 1));
        SMH_TRY(run.h_sc.alloc(sizeof(CgScalars<T>), hipHostMallocDefault));
        T *xd = (T *)x->d.get();
        const T *bd = (const T *)b->d.get();
        // R = B - A X  (:38) ; P = R.clone() (:39) ; rr_c = r_c . r_c (:40).  K1m's own statuses are decided here, before any launch.
        SMH_TRY(smh_crs_spmv_many_dev(m, xd, n, r.get(), k, ld, s));
        SMH_TRY(mv_rsub_into(m->dtype, r.get(), bd, n, ld, s));
        if (n) SMH_HIP(hipMemcpyAsync(p.get(), r.get(), n * ld * sizeof(T), hipMemcpyDeviceToDevice, s));
        unsigned nb2 = 0;
        SMH_TRY(mv_dot_partials(m->dtype, r.get(), r.get(), n, ld, rr_part.get(), &nb2, s));
        hipLaunchKernelGGL(k_cgm_init<T>, dim3((unsigned)(ld < 1024 ? ld : 1024)), dim3(kBlock), 0, s, sc.get(), rr_part.get(), nb, (uint32_t)k, (uint32_t)ld, tol,
                           (uint64_t)iter_max);
        SMH_HIP(hipGetLastError());
        auto body = [&]() -> int {
            SMH_TRY(smh_crs_spmv_many_dev(m, p.get(), n, ap.get(), k, ld, s));                                             // :43
            SMH_TRY(mv_dot_partials(m->dtype, p.get(), ap.get(), n, ld, pap_part.get(), &nb2, s));
            hipLaunchKernelGGL(k_cgm_update<T>, dim3(gx, nb), dim3(kBlock), 0, s, sc.get(), sc2.get(), pap_part.get(), nb, r.get(), ap.get(), (uint64_t)n,
                               (uint32_t)ngroups, (uint32_t)k, rr_part.get());                                              // :45, :49-51
            hipLaunchKernelGGL(k_cgm_p<T>, dim3(gx, pb), dim3(kBlock), 0, s, sc2.get(), sc.get(), rr_part.get(), nb, p.get(), r.get(), xd, (uint64_t)n,
                               (uint32_t)ngroups);                                                                          // :47, :51-59
            SMH_HIP(hipGetLastError());
            return SMH_OK;
        };
        SMH_TRY(run.loop(m->dtype, iter_max, check_every, body, sc.get()));
        // the per-column scalars, once
        SMH_HIP(hipMemcpyAsync(h_all.data(), sc.get(), (ld + 1) * sizeof(CgScalars<T>), hipMemcpyDeviceToHost, s));
        SMH_HIP(hipStreamSynchronize(s));
        return SMH_OK;
    }, nullptr, nullptr);
    if (rc != SMH_OK) return rc;
    for (size_t c = 0; c < k; ++c) {
        iters_out[c] = (size_t)h_all[1 + c].iters;
        rr_out[c] = (double)h_all[1 + c].rr;
    }
    return SMH_OK;
}

int cg_solve_many(smh_crs *m, const smh_mvec *b, smh_mvec *x, double tol, size_t iter_max, size_t check_every, size_t *iters_out, double *rr_out) {
    if (m->dtype == SMH_F64) return cg_solve_many_t<double>(m, b, x, tol, iter_max, check_every, iters_out, rr_out);
    return cg_solve_many_t<float>(m, b, x, tol, iter_max, check_every, iters_out, rr_out);
}

}  // namespace smh

using namespace smh;

extern "C" {

// ---- the entry points: ConjugateGradient on k right-hand sides at once -------------------------------------------------------------
int smh_cg_solve_many(smh_crs *m, const smh_mvec *b, smh_mvec *x, double tol, size_t iter_max, size_t check_every, size_t *iters_out,
                      double *rr_out) {
    if (!m || !b || !x) return fail(SMH_ERR_INVALID, "NULL handle");
    if (!iters_out || !rr_out) return fail(SMH_ERR_INVALID, "NULL output array");
    SMH_TRY(check_solve_vec(m, b, x, "multi-vector dtype differs from the matrix's", /*refuse_aliased*/ true, &check_every, kCgCheckEvery));
    return cg_solve_many(m, b, x, tol, iter_max, check_every, iters_out, rr_out);
}

int smh_cg_solve_many_host(smh_crs *m, const void *b_host, size_t n, size_t k, void *x_host_inout, double tol, size_t iter_max,
                           size_t *iters_out, double *rr_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (!iters_out || !rr_out) return fail(SMH_ERR_INVALID, "NULL output array");
    SMH_TRY(check_solve_host(m, b_host, n, x_host_inout, n, /*null_vectors*/ true, /*refuse_aliased*/ false));
    smh_mvec *b = nullptr, *x = nullptr;
    int rc = smh_mvec_from_host((smh_dtype)m->dtype, n, k, b_host, &b);
    if (rc == SMH_OK) rc = smh_mvec_from_host((smh_dtype)m->dtype, n, k, x_host_inout, &x);
    if (rc == SMH_OK) rc = smh_cg_solve_many(m, b, x, tol, iter_max, 0, iters_out, rr_out);
    if (rc == SMH_OK && n) rc = smh_mvec_download(x, x_host_inout);
    smh_mvec_destroy(b);
    smh_mvec_destroy(x);
    return rc;
}

}  // extern "C"
