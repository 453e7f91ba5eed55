// precond.hpp -- the preconditioner object of the preconditioned solvers (pcg.hip: Jacobi-, SGS-, ILU- and FSAI-PCG; gmres.hip and bicgstab.hip: the
// right-preconditioned GMRES and BiCGSTAB).  Precond says what M^-1 is -- nothing, a division by the diagonal, two triangular solves on one handle, two
// products on two -- and everything that depends on that sits here: how a driver's template applies it (PrecondShape), the checks of its handles, its
// set-up on the device, its application and the nodes that takes in a captured batch, whose budget is here too.
#pragma once
#include "internal.hpp"
#include "solver_host.hpp"
#include "solver_tree.hpp"

#include <cstdlib>
#include <type_traits>

namespace smh {

// what the preconditioned entry points (smh_gmres_precond_solve*, smh_bicgstab_precond_solve*) decide about `precond` and `f` before
// anything else
inline int check_precond(int precond, const smh_crs *f) {
    if (precond < SMH_PRECOND_NONE || precond > SMH_PRECOND_ILU) return fail(SMH_ERR_INVALID, "precond is %d: it must be one of SMH_PRECOND_*", precond);
    if (precond == SMH_PRECOND_ILU && !f) return fail(SMH_ERR_INVALID, "NULL handle");
    if (precond != SMH_PRECOND_ILU && f) return fail(SMH_ERR_INVALID, "a factor handle goes with SMH_PRECOND_ILU alone");
    return SMH_OK;
}

// d[i] = get(i, i); *bad = the smallest row whose diagonal entry is zero or absent (stays ~0 when there is none)
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_pcg_diag(const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val, uint64_t n, T *__restrict__ d,
           unsigned long long *bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        T v = T(0);
        for (uint64_t q = off[i]; q < off[i + 1]; ++q)
            if (col[q] == i) { v = val[q]; break; }
        d[i] = v;
        if (v == T(0)) atomicMin(bad, (unsigned long long)i);
    }
}

// d[i] = get(i, i) of h, on s once h's own stream has finished, and the verdict: a zero or absent diagonal entry cannot be divided by
// (name: whose refusal it is; d_bad: one word of scratch)
template <typename T>
int probe_diagonal(const smh_crs *h, size_t n, T *d, unsigned long long *d_bad, const char *name, hipStream_t s) {
    SMH_HIP(hipStreamSynchronize(h->stream));  // (the handle is read on another stream than the one that wrote it)
    unsigned long long bad = ~0ull;
    SMH_HIP(hipMemcpyAsync(d_bad, &bad, sizeof bad, hipMemcpyHostToDevice, s));
    if (n) hipLaunchKernelGGL((k_pcg_diag<T>), dim3(pcg_grid(n) * 4), dim3(kBlock), 0, s, h->d_off, h->d_col, (const T *)h->d_val, (uint64_t)n, d, d_bad);
    SMH_HIP(hipGetLastError());
    SMH_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    SMH_HIP(hipStreamSynchronize(s));
    if (bad != ~0ull) return fail(SMH_ERR_INVALID, "%s: zero or absent diagonal entry in row %llu", name, bad);
    return SMH_OK;
}

// most nodes of a captured batch (a linear chain): beyond it the bodies per batch go down, and a single body beyond it runs
// uncaptured.  How the bodies reach the device changes no bit.  SMH_SGS_GRAPH_NODES: tuning knob
inline size_t batch_node_budget() {
    if (const char *e = getenv("SMH_SGS_GRAPH_NODES")) return (size_t)strtoull(e, nullptr, 10);
    return 4096;
}

// M^-1 by its kind, z = M^-1 r.
// Diagonal: z_i = r_i / d_i, d_i the first stored (i, i) of the matrix f (Jacobi) -- a division inside the solver's own sweeps.
// Solves: two triangular solves on the handle f through n values of scratch, z = T_upper^-1 (scale(T_lower^-1 r)): SGS on the
// matrix itself, both diagonals stored, the right-hand side of the upper solve scaled by the diagonal; ILU(0) on the factor handle
// (ilu.hip), the lower solve with the unit diagonal, no scaling.
// Products: two products on two handles, z = gt (f r): FSAI's pair (fsai.hip), each by the handle's own AUTO kernel.
struct Precond {
    enum Kind { None, Diagonal, Solves, Products } kind;
    const char *name;  // whose refusal a refusal is
    smh_crs *f;
    struct SolveForm {
        int lower_diag;
        bool scale_rhs;
    };
    union {  // by kind: Solves' form, Products' second handle
        SolveForm solve;
        smh_crs *gt;
    };
};
constexpr const char *kFsaiName = "FSAI preconditioner";
inline Precond no_precond() { return {Precond::None, "no preconditioner", nullptr, {}}; }
inline Precond jacobi_precond(smh_crs *m) { return {Precond::Diagonal, "Jacobi preconditioner", m, {}}; }
inline Precond sgs_precond(smh_crs *m) { return {Precond::Solves, "SGS preconditioner", m, {{SMH_DIAG_NON_UNIT, true}}}; }
inline Precond ilu_precond(smh_crs *f) { return {Precond::Solves, "ILU preconditioner", f, {{SMH_DIAG_UNIT, false}}}; }
inline Precond fsai_precond(smh_crs *g, smh_crs *gt) {
    Precond pc{Precond::Products, kFsaiName, g, {}};
    pc.gt = gt;
    return pc;
}
// SMH_PRECOND_* on the matrix m and ILU's factor f (check_precond has passed)
inline Precond precond_of(int precond, smh_crs *m, smh_crs *f) {
    switch (precond) {
    case SMH_PRECOND_JACOBI: return jacobi_precond(m);
    case SMH_PRECOND_SGS: return sgs_precond(m);
    case SMH_PRECOND_ILU: return ilu_precond(f);
    default: return no_precond();
    }
}

// How a driver's template applies M^-1: not at all, inside its own sweeps, or by launches of the preconditioner's own (solves
// and products alike: a vector in, a vector out, n values of scratch)
enum PrecondShape { kPcNone, kPcFused, kPcLaunched };
inline PrecondShape precond_shape(const Precond &pc) {
    return pc.kind == Precond::None ? kPcNone : pc.kind == Precond::Diagonal ? kPcFused : kPcLaunched;
}

// go(T(), shape) with T the type of dtype and shape an std::integral_constant of PrecondShape: where a driver template of both is
// instantiated, all six from the one expression in go
template <typename Go> int with_dtype_and_shape(int dtype, PrecondShape shape, Go &&go) {
    auto typed = [&](auto t) -> int {
        switch (shape) {
        case kPcNone: return go(t, std::integral_constant<PrecondShape, kPcNone>());
        case kPcFused: return go(t, std::integral_constant<PrecondShape, kPcFused>());
        default: return go(t, std::integral_constant<PrecondShape, kPcLaunched>());
        }
    };
    return dtype == SMH_F64 ? typed(double()) : typed(float());
}

// What a solver refuses of the preconditioner's handles after its entry point's argument checks: solves and products read the
// stored entries, so an orphaned one (the first push of a replay) is refused
inline int precond_check_handles(const Precond &pc) {
    const bool reads = pc.kind == Precond::Solves || pc.kind == Precond::Products;
    if (reads && (pc.f->orphans || (pc.kind == Precond::Products && pc.gt->orphans)))
        return fail(SMH_ERR_INVALID, "%s: the handle holds an orphaned entry", pc.name);
    return SMH_OK;
}

// z = M^-1 r on stream s (w: n values of scratch; z may be r; precond_prepare has run).  active gates the solves' launches; the
// products run ungated, as the body's own does: past the stop they form the same z from the same r again
inline int precond_apply_enqueue(const Precond &pc, const void *r, void *w, void *z, const uint32_t *active, hipStream_t s) {
    if (pc.kind == Precond::Products) {
        SMH_TRY(spmv_enqueue(pc.f, r, pc.f->n_rows, w, SMH_SPMV_AUTO, s));
        return spmv_enqueue(pc.gt, w, pc.f->n_rows, z, SMH_SPMV_AUTO, s);
    }
    SMH_TRY(trisolve_enqueue(pc.f, SMH_TRI_LOWER, pc.solve.lower_diag, false, r, w, active, s));
    return trisolve_enqueue(pc.f, SMH_TRI_UPPER, SMH_DIAG_NON_UNIT, pc.solve.scale_rhs, w, z, active, s);
}

// y = M x in storage order when *gate != 0, nothing at all otherwise: k_spmv_seq's operations (one lane per row, the product rounded,
// then added: SMH_SPMV_SEQ's bits) behind a device word.  For an application that is due in few bodies of a captured batch (GMRES's
// cycle end), where the handle's own ungated product would run, and cost, in every body.  Columns < the length of x: precond_prepare
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_gated_seq(const uint32_t *__restrict__ gate, const uint32_t *__restrict__ off, const uint32_t *__restrict__ col, const T *__restrict__ val,
            const T *__restrict__ x, T *__restrict__ y, uint64_t n_rows) {
    if (!*gate) return;  // block-uniform
    for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t e = off[row + 1];
        T sum = T(0);
        for (uint64_t k = off[row]; k < e; ++k) sum = p_add(sum, p_mul(x[col[k]], val[k]));
        y[row] = sum;
    }
}

inline int gated_seq_enqueue(const smh_crs *h, const void *x, void *y, const uint32_t *gate, hipStream_t s) {
    const size_t n = h->n_rows;
    if (!n) return SMH_OK;
    size_t blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 8192) blocks = 8192;
    if (h->dtype == SMH_F64)
        hipLaunchKernelGGL((k_gated_seq<double>), dim3((unsigned)blocks), dim3(kBlock), 0, s, gate, h->d_off, h->d_col, (const double *)h->d_val, (const double *)x,
                           (double *)y, (uint64_t)n);
    else
        hipLaunchKernelGGL((k_gated_seq<float>), dim3((unsigned)blocks), dim3(kBlock), 0, s, gate, h->d_off, h->d_col, (const float *)h->d_val, (const float *)x,
                           (float *)y, (uint64_t)n);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// z = M^-1 r when *gate != 0 and no work otherwise (w: n values of scratch; z may be r; gate: a device word).  The solves as above;
// the pair by two gated storage-order products, w = G r and z = G^T w with SMH_SPMV_SEQ's bits -- not the handles' AUTO kernels
inline int precond_apply_gated_enqueue(const Precond &pc, const void *r, void *w, void *z, const uint32_t *gate, hipStream_t s) {
    if (pc.kind != Precond::Products) return precond_apply_enqueue(pc, r, w, z, gate, s);
    // SMH_FSAI_END_GATE=0 (tuning knob, for measuring what the gate saves): the handles' own ungated products instead -- AUTO's bits
    if (const char *e = getenv("SMH_FSAI_END_GATE")) {
        if (atoi(e) == 0) return precond_apply_enqueue(pc, r, w, z, gate, s);
    }
    SMH_TRY(gated_seq_enqueue(pc.f, r, w, gate, s));
    return gated_seq_enqueue(pc.gt, w, z, gate, s);
}

// the launches of one application (precond_prepare has run); a product: a few nodes at most
inline size_t precond_apply_nodes(const Precond &pc) {
    if (pc.kind == Precond::Products) return 2 * 4;
    return pc.f->tri[SMH_TRI_LOWER].launches.size() + pc.f->tri[SMH_TRI_UPPER].launches.size();
}

// the checks of a preconditioner's handles that need the device, before a solve's first launch: columns; the solves' schedules (a
// stored diagonal in every row is the caller's to ask of them).  None and Diagonal read no handle's columns: nothing
inline int precond_prepare(const Precond &pc) {
    if (pc.kind == Precond::None || pc.kind == Precond::Diagonal) return SMH_OK;
    SMH_TRY(columns_within_n_cols(pc.f, pc.name));
    if (pc.kind == Precond::Products) return columns_within_n_cols(pc.gt, pc.name);
    SMH_TRY(ensure_tri_schedule(pc.f, SMH_TRI_LOWER));
    return ensure_tri_schedule(pc.f, SMH_TRI_UPPER);
}

// What a solve does about its preconditioner on its own stream s after its allocations (ws: the run's) and before its first launch.
// Diagonal: diag (n values) takes the matrix's diagonal and keeps it, a zero or absent entry is refused.  Solves: the same probe of
// the handle the solves run on; the solves read the handle's values, so what diag (any n values of scratch) took is not kept.
// Products: nothing divides by a factor's value, so nothing is probed; both handles' AUTO forms are built here, outside any capture,
// and their streams drained (the handles are read on another stream than the ones that wrote them).
template <typename T>
int precond_setup(const Precond &pc, size_t n, T *diag, Scratch &ws, hipStream_t s) {
    if (pc.kind == Precond::None) return SMH_OK;
    unsigned long long *d_bad = nullptr;
    SMH_TRY(ws.alloc(&d_bad, 1));
    if (pc.kind != Precond::Products) return probe_diagonal(pc.f, n, diag, d_bad, pc.name, s);
    SMH_TRY(smh_crs_prepare(pc.f, SMH_SPMV_AUTO));
    return smh_crs_prepare(pc.gt, SMH_SPMV_AUTO);
}

// z = M^-1 r alone, by the handle's stream (smh_crs_{sgs,ilu,fsai}_apply_vec; what: the caller's name); r and z: n values each on
// the device, equal or disjoint
inline int precond_apply_vec(const Precond &pc, const smh_vec *r, smh_vec *z, const char *what) {
    smh_crs *f = pc.f;
    if (r->dtype != f->dtype || z->dtype != f->dtype) return fail(SMH_ERR_INVALID, "%s", kVecDtype);
    if (f->n_rows != f->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    if (f->n_rows != r->n || f->n_rows != z->n) return fail(SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch");
    SMH_TRY(precond_check_handles(pc));
    if (pc.kind == Precond::Products) {
        SMH_TRY(ilu_check_pair(f, pc.gt, pc.name));
        SMH_HIP(hipStreamSynchronize(pc.gt->stream));  // (gt is read on g's stream)
    }
    const size_t n = f->n_rows, bytes = n * dtype_size(f->dtype);
    const char *pr = (const char *)r->d, *pz = (const char *)z->d;
    if (pr != pz && pr < pz + bytes && pz < pr + bytes) return fail(SMH_ERR_INVALID, "%s: r and z overlap in part", what);
    SMH_TRY(precond_prepare(pc));
    if (pc.kind == Precond::Solves && f->tri[SMH_TRI_LOWER].first_no_diag != ~0ull)
        return fail(SMH_ERR_INVALID, "%s: no diagonal entry stored in row %llu", pc.name, (unsigned long long)f->tri[SMH_TRI_LOWER].first_no_diag);
    Scratch scr;
    char *w = nullptr;
    SMH_TRY(scr.alloc(&w, bytes));
    const hipStream_t s = f->stream;
    const int rc = precond_apply_enqueue(pc, r->d, w, z->d, nullptr, s);
    if (rc != SMH_OK) return keep_error(rc, [&] { (void)hipStreamSynchronize(s); (void)hipGetLastError(); });
    SMH_HIP(hipStreamSynchronize(s));  // (before the scratch goes back to the pool)
    return SMH_OK;
}

// The bodies of a captured batch under the node budget, per_body nodes each: check_every, fewer when that many are beyond the
// budget, one when a single body is (*capture: whether a batch is captured at all).
inline size_t bodies_within_budget(size_t per_body, size_t check_every, bool *capture) {
    const size_t budget = batch_node_budget();
    size_t bodies = check_every;
    if (per_body * bodies > budget) bodies = budget / per_body ? budget / per_body : 1;
    *capture = per_body <= budget;
    return bodies;
}

}  // namespace smh
