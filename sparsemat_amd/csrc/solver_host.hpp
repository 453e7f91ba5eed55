// solver_host.hpp -- what the host side of the device-resident solvers shares (cg.hip, cg_many.hip, pcg.hip, bicgstab.hip, gmres.hip, eigsh.hip and their
// entry points): the argument checks of the entry points and the skeleton of a solve around solve_in_batches (internal.hpp).
// A solver is its allocations, its set-up launches, a body lambda and SolveRun::run; the kernels are its own file's.
#pragma once
#include "internal.hpp"

namespace smh {

// ---- the argument checks of the entry points, decided before any launch -------------------------------------------------------------
constexpr const char *kVecDtype = "vector dtype differs from the matrix's";  // (smh_cg_solve_vec and smh_cg_solve_many word it in their own ways)
// check_every = 0 stands for 4 bodies per poll in smh_cg_solve* (cg.hip, cg_many.hip); 8 in the preconditioned solvers and BiCGSTAB
constexpr size_t kCgCheckEvery = 4;

// what a matrix a and a factor f of it (ILU(0)'s, or one of FSAI's two: name) must agree in
inline int ilu_check_pair(const smh_crs *a, const smh_crs *f, const char *name = "ILU preconditioner") {
    if (a->n_rows != a->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    if (f->n_rows != f->n_cols) return fail(SMH_ERR_NOT_SQUARE, "%s: the factor is not square", name);
    if (f->n_rows != a->n_rows) return fail(SMH_ERR_DIM_MISMATCH, "%s: the factor's dimension differs from the matrix's", name);
    if (f->dtype != a->dtype) return fail(SMH_ERR_INVALID, "%s: the factor's dtype differs from the matrix's", name);
    if (f->device != a->device) return fail(SMH_ERR_INVALID, "%s: the factor and the matrix live on different devices", name);
    return SMH_OK;
}

inline bool same_storage(const smh_vec *b, const smh_vec *x) { return b == x || (b->d && b->d == x->d); }
inline bool same_storage(const smh_mvec *b, const smh_mvec *x) { return b == x || b->d.get() == x->d.get(); }
inline bool same_columns(const smh_vec *, const smh_vec *) { return true; }
inline bool same_columns(const smh_mvec *b, const smh_mvec *x) { return b->k == x->k; }

// The _vec form (V: smh_vec, or smh_mvec for the k-column CG), in the order of the reports.  Where the entry points differ
// ("known inconsistencies of the solvers' checks") the caller says so: the text of the dtype refusal, whether b and x
// in one storage are refused, and how many bodies per poll check_every = 0 stands for.  factor: ILU's, or FSAI's G (factor_name says
// whose), checked against m where the others check that m is square.
template <typename V>
int check_solve_vec(const smh_crs *m, const V *b, const V *x, const char *dtype_message, bool refuse_aliased, size_t *check_every,
                    size_t default_check_every, const smh_crs *factor = nullptr, const char *factor_name = "ILU preconditioner") {
    if (!m || !b || !x) return fail(SMH_ERR_INVALID, "NULL handle");
    if (b->dtype != m->dtype || x->dtype != m->dtype) return fail(SMH_ERR_INVALID, "%s", dtype_message);
    if (refuse_aliased && same_storage(b, x)) return fail(SMH_ERR_INVALID, "b and x are the same storage");
    if (factor) SMH_TRY(ilu_check_pair(m, factor, factor_name));
    else if (m->n_rows != m->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");  // linearsolver.rs:30-32
    if (m->n_rows != b->n || m->n_rows != x->n || !same_columns(b, x))
        return fail(SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch");  // :33-36
    if (*check_every == 0) *check_every = default_check_every;
    return SMH_OK;
}

// The host form.  null_vectors: the entry point refuses a NULL vector of n > 0 itself (smh_cg_solve leaves that to the upload);
// refuse_aliased: ... and b_host == x_host (smh_bicgstab_solve and smh_gmres_solve alone).
inline int check_solve_host(const smh_crs *m, const void *b_host, size_t b_len, const void *x_host, size_t x_len, bool null_vectors,
                            bool refuse_aliased, const smh_crs *factor = nullptr, const char *factor_name = "ILU preconditioner") {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    const size_t n = m->n_rows;
    if (factor) SMH_TRY(ilu_check_pair(m, factor, factor_name));
    else if (n != m->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    if (n != b_len || n != x_len) return fail(SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch");
    if (null_vectors && n && (!b_host || !x_host)) return fail(SMH_ERR_INVALID, "NULL host vector");
    if (refuse_aliased && n && b_host == x_host) return fail(SMH_ERR_INVALID, "b and x are the same storage");
    return SMH_OK;
}

// A pair of factor handles in place of one (FSAI's g and gt: name): a NULL one first, as a NULL matrix; then the checks above with g
// the factor; gt against m after everything else
template <typename V>
int check_pair_vec(const smh_crs *m, const smh_crs *g, const smh_crs *gt, const char *name, const V *b, const V *x, size_t *check_every,
                   size_t default_check_every) {
    if (!g || !gt) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(check_solve_vec(m, b, x, kVecDtype, /*refuse_aliased*/ true, check_every, default_check_every, g, name));
    return ilu_check_pair(m, gt, name);
}

inline int check_pair_host(const smh_crs *m, const smh_crs *g, const smh_crs *gt, const char *name, const void *b_host, size_t b_len,
                           const void *x_host, size_t x_len, bool refuse_aliased) {
    if (!g || !gt) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(check_solve_host(m, b_host, b_len, x_host, x_len, /*null_vectors*/ true, refuse_aliased, g, name));
    return ilu_check_pair(m, gt, name);
}

// GMRES's restart length, after the checks above: 0 stands for default_restart, anything above max_restart is refused
inline int check_solve_restart(size_t *restart, size_t default_restart, size_t max_restart) {
    if (*restart == 0) *restart = default_restart;
    if (*restart > max_restart) return fail(SMH_ERR_INVALID, "restart is %zu: it must be at most %zu (0: the default, %zu)", *restart, max_restart, default_restart);
    return SMH_OK;
}

// ---- the skeleton of a solve --------------------------------------------------------------------------------------------------------
// What a driver takes after the matrix and the preconditioner: an entry point fills it from its argument list, nobody else writes one
// out.  b and x: n values each of the matrix's dtype, in host or device memory; x is the start and is written once, after the loop.
// The out-parameters are optional and written when the solve succeeded.
struct SolveCall {
    const void *b;
    void *x;
    size_t n;
    double tol;
    size_t iter_max;
    int variant;
    size_t check_every;
    size_t *iters_out;
    double *rr_out;
    int *breakdown_out = nullptr;  // BiCGSTAB and GMRES
    size_t restart = 0;            // GMRES (check_solve_restart has passed)
    size_t *cycles_out = nullptr;  // GMRES
};

// The stream a solve runs on -- the handle's (CG, the k-column CG) or one of its own, created on demand (the others) --, its device
// workspaces, the pinned block that solve_in_batches polls through, and the scalar block as the last poll saw it.
class SolveRun {
    Stream own_;  // (declared first: the workspaces go before their stream does)

  public:
    Scratch ws;
    PinnedBuf h_sc;
    int converged = 0;
    size_t iters = 0;
    double rr = 0.0;
    hipStream_t s = nullptr;

    SolveRun() = default;                                         // a stream of its own: own_stream()
    explicit SolveRun(hipStream_t on) : s(on), live_(true) {}    // the handle's
    int own_stream() {
        SMH_TRY(own_.create());
        s = own_.get();
        live_ = true;
        return SMH_OK;
    }

    // up to iter_max bodies in batches of check_every (solve_in_batches, internal.hpp); d_sc: the device block in CgScalars' layout
    template <typename Body>
    int loop(int dtype, size_t iter_max, size_t check_every, Body &&body, const void *d_sc, bool capture = true) {
        return solve_in_batches(dtype, s, iter_max, check_every, body, d_sc, h_sc.get(), &converged, &iters, &rr, capture);
    }

    // go(): the whole solve.  iters_out / rr_out (optional) are written when it succeeded.
    template <typename Go> int run(Go &&go, size_t *iters_out, double *rr_out) {
        // the stream is drained before the workspaces go back to the pool (which hands them straight to the next caller), also when
        // the solve failed half way
        const int rc = keep_error(go(), [&] {
            if (live_) (void)hipStreamSynchronize(s);
            (void)hipGetLastError();
        });
        if (rc != SMH_OK) return rc;
        if (iters_out) *iters_out = iters;
        if (rr_out) *rr_out = rr;
        return SMH_OK;
    }

  private:
    bool live_ = false;
};

// What opens a solve on a stream s of its own: waits for the matrix's stream (the matrix is read on another stream than the one
// that wrote it), stages b into r and the start into x -- b_in / x_io: n values each in host or device memory, the copies are
// hipMemcpyDefault -- and forms r = b - A x (ax: n values of scratch).  This is the solve's first product: it comes before any
// capture, and the handle's lazy workspaces exist from here on.
template <typename T>
int stage_residual(smh_crs *m, int variant, const T *b_in, const T *x_io, size_t n, T *r, T *x, T *ax, hipStream_t s) {
    SMH_HIP(hipStreamSynchronize(m->stream));
    if (n) {
        SMH_HIP(hipMemcpyAsync(r, b_in, n * sizeof(T), hipMemcpyDefault, s));
        SMH_HIP(hipMemcpyAsync(x, x_io, n * sizeof(T), hipMemcpyDefault, s));
    }
    SMH_TRY(spmv_enqueue(m, x, n, ax, variant, s));
    if (n) SMH_TRY(launch_ew(sizeof(T) == 8 ? SMH_F64 : SMH_F32, Ew::Sub, r, ax, n, 0.0, nullptr, s));
    return SMH_OK;
}

}  // namespace smh
