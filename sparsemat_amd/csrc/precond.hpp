// precond.hpp -- what the preconditioned solvers share (pcg.hip: Jacobi-, SGS-, ILU- and FSAI-PCG; gmres.hip and bicgstab.hip: the right-preconditioned
// GMRES and BiCGSTAB): what their entry points decide about `precond` and `f`, the probe of a handle's diagonal, the preconditioner applied by two triangular solves on one handle or by two products on two (Precond) and the
// node budget of a captured batch that holds such applications.
#pragma once
#include "internal.hpp"
#include "solver_tree.hpp"

#include <cstdlib>

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
inline size_t sgs_graph_nodes() {
    if (const char *e = getenv("SMH_SGS_GRAPH_NODES")) return (size_t)strtoull(e, nullptr, 10);
    return 4096;
}

// A preconditioner applied by two sweeps over handles of the factor's kind, z = M^-1 r through n values of scratch w.
// Two triangular solves on one handle (gt == nullptr), z = T_upper^-1 (scale(T_lower^-1 r)): SGS on the matrix itself, both
// diagonals stored, the right-hand side of the upper solve scaled by the diagonal; ILU(0) on the factor handle (ilu.hip), the lower
// solve with the unit diagonal, no scaling.  Two products on two handles (gt != nullptr), z = G^T (G r): FSAI (fsai.hip), each by the
// handle's own AUTO kernel.
struct Precond {
    smh_crs *f;
    int lower_diag;
    bool scale_rhs;
    const char *name;
    smh_crs *gt = nullptr;
};
inline Precond sgs_precond(smh_crs *m) { return {m, SMH_DIAG_NON_UNIT, true, "SGS preconditioner"}; }
inline Precond ilu_precond(smh_crs *f) { return {f, SMH_DIAG_UNIT, false, "ILU preconditioner"}; }
inline Precond fsai_precond(smh_crs *g, smh_crs *gt) { return {g, SMH_DIAG_NON_UNIT, false, "FSAI preconditioner", gt}; }

// z = M^-1 r on stream s (w: n values of scratch; z may be r; precond_prepare has run).  active gates the solves' launches; the
// products run ungated, as the body's own does: past the stop they form the same z from the same r again
inline int precond_apply_enqueue(const Precond &pc, const void *r, void *w, void *z, const uint32_t *active, hipStream_t s) {
    if (pc.gt) {
        SMH_TRY(spmv_enqueue(pc.f, r, pc.f->n_rows, w, SMH_SPMV_AUTO, s));
        return spmv_enqueue(pc.gt, w, pc.f->n_rows, z, SMH_SPMV_AUTO, s);
    }
    SMH_TRY(trisolve_enqueue(pc.f, SMH_TRI_LOWER, pc.lower_diag, false, r, w, active, s));
    return trisolve_enqueue(pc.f, SMH_TRI_UPPER, SMH_DIAG_NON_UNIT, pc.scale_rhs, w, z, active, s);
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
    if (!pc.gt) return precond_apply_enqueue(pc, r, w, z, gate, s);
    // SMH_FSAI_END_GATE=0 (tuning knob, for measuring what the gate saves): the handles' own ungated products instead -- AUTO's bits
    if (const char *e = getenv("SMH_FSAI_END_GATE")) {
        if (atoi(e) == 0) return precond_apply_enqueue(pc, r, w, z, gate, s);
    }
    SMH_TRY(gated_seq_enqueue(pc.f, r, w, gate, s));
    return gated_seq_enqueue(pc.gt, w, z, gate, s);
}

// the launches of one application (precond_prepare has run); a product: a few nodes at most
inline size_t precond_apply_nodes(const Precond &pc) {
    if (pc.gt) return 2 * 4;
    return pc.f->tri[SMH_TRI_LOWER].launches.size() + pc.f->tri[SMH_TRI_UPPER].launches.size();
}

// the checks of a preconditioner's handles that need the device: columns; the solves' schedules (a stored diagonal in every row is
// the caller's to ask of them)
inline int precond_prepare(const Precond &pc) {
    SMH_TRY(columns_within_n_cols(pc.f, pc.name));
    if (pc.gt) return columns_within_n_cols(pc.gt, pc.name);
    SMH_TRY(ensure_tri_schedule(pc.f, SMH_TRI_LOWER));
    return ensure_tri_schedule(pc.f, SMH_TRI_UPPER);
}

// The bodies of a captured batch under the node budget, per_body nodes each: check_every, fewer when that many are beyond the
// budget, one when a single body is (*capture: whether a batch is captured at all).
inline size_t bodies_within_budget(size_t per_body, size_t check_every, bool *capture) {
    const size_t budget = sgs_graph_nodes();
    size_t bodies = check_every;
    if (per_body * bodies > budget) bodies = budget / per_body ? budget / per_body : 1;
    *capture = per_body <= budget;
    return bodies;
}

}  // namespace smh
