// pcg.hip -- Jacobi-preconditioned conjugate gradient, gfx950.
//
// An EXTENSION: the reference's only solver is the unpreconditioned ConjugateGradient (linearsolver.rs:12-61).  This is
// that recurrence with z = r / diag(A), diag_i = get(i, i) (first match in storage order: sparsemat_crs.rs:54-67,
// 136-142) -- same guards (:30-36), same stop rule (sqrt(f64(r.r)) < tol after the update of r, before beta, :52-54),
// same arithmetic conventions (one rounding per operation; multiply and add never contracted):
//   r = b - A x;  p = r / d;  rz = r.(r/d)
//   loop: Ap = A p;  alpha = rz / (p.Ap);  x += p*alpha;  r -= Ap*alpha;  rr = r.r;  stop test;
//         rz' = r.(r/d);  beta = rz' / rz;  p = p*beta + r/d
// Kernels: the SpMV is the matrix's own (K1r/K1s/...); the tail is fused so that z is never stored: one sweep updates
// r and leaves the block partials of r.r and r.(r/d) (r, Ap, d in; r out), one sweep adds p*alpha to x and rebuilds p
// (p, x, r, d in; p, x out): 10 n values per iteration beside the SpMV (the plain CG moves 8 n; the two reads of d are
// what the preconditioner costs), p.Ap out of the SpMV epilogue when the kernel offers it.  All scalars (r.r, r.z, p.Ap,
// alpha, beta, the stop flag, the iteration count) live in device memory as in cg.hip: the host replays a hipGraph of 8
// bodies and polls one small block per batch (solve_in_batches, internal.hpp) -- no synchronisation inside an iteration.
// The sweeps state their arithmetic once, on solver_tree.hpp's sweep; the sums and the one-workgroup folds of their partials are
// its tree (block_sums / block_sum1, fold1 / fold2) -- deterministic.
// The second half of the file is the same recurrence with a preconditioner that is applied by launches of its own (Precond,
// precond.hpp), where z is a vector; the scalars, k_pcg_alpha and the sums are these.  Symmetric Gauss-Seidel (smh_pcg_sgs_solve*,
// smh_crs_sgs_apply_vec) is two level-scheduled triangular solves (trisolve.hip) on the matrix itself, ILU(0) (smh_pcg_ilu_solve*,
// smh_crs_ilu_apply_vec) the same on a factor handle (ilu.hip), FSAI (smh_pcg_fsai_solve*, smh_crs_fsai_apply_vec; fsai.hip)
// z = G^T (G r) by two products of a pair of factor handles' own kernels.
// Host side: both drivers (pcg_t, pcg_launched_t) are their allocations, their set-up launches, a body lambda and SolveRun::run
// (solver_host.hpp: the stream, the workspaces, the drain, r = b - A x); Precond, its set-up (the zero-diagonal probe) and the node
// budget of a captured batch are precond.hpp's (shared with gmres.hip and bicgstab.hip), the source of p.Ap one function here
// (pap_source); the entry points' argument checks are solver_host.hpp's.
#include "internal.hpp"
#include "precond.hpp"
#include "solver_host.hpp"
#include "solver_tree.hpp"

#include <cmath>
#include <cstring>

using namespace smh;

namespace smh {
unsigned reduce_blocks(size_t n);  // blas1.hip
}

namespace {

// ---- device-resident scalars (like cg.hip): nothing of an iteration passes through the host ---------------------------
template <typename T>
struct PcgScalars {
    T rr, rz, pap, alpha, beta;
    uint32_t converged;
    uint32_t active;   // this loop body runs (not converged, fewer than iter_max bodies entered)
    uint32_t entered;  // ... was entered: its x update is due even if the stop test then ends the loop
    uint32_t pad_;
    uint64_t iters;
    uint64_t iter_max;
    double tol;
};
static_assert(scalars_like_cg<PcgScalars>(), "PcgScalars and CgScalars have drifted apart");  // (the host polls it through CG's reader)

template <typename T>
__global__ void k_pcg_init(PcgScalars<T> *sc, double tol, uint64_t iter_max) {
    sc->rr = sc->rz = sc->pap = sc->alpha = sc->beta = T(0);
    sc->converged = sc->active = sc->entered = sc->pad_ = 0;
    sc->iters = 0;
    sc->iter_max = iter_max;
    sc->tol = tol;
}

// out[b] = sum of block b's strided share of in[0..n): first stage of folding the SpMV epilogue's per-tile partials
template <typename T>
__global__ void __launch_bounds__(kBlock) k_pcg_sum_stage1(const T *__restrict__ in, uint64_t n, T *__restrict__ out) {
    block_partial(strided_sum(in, n, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x), out);
}

// p.Ap = fold(partials); decide whether this body runs; alpha = r.z / p.Ap
template <typename T>
__global__ void __launch_bounds__(kBlock) k_pcg_alpha(PcgScalars<T> *sc, const T *__restrict__ partials, uint32_t count) {
    const T pap = fold1(partials, count);
    if (threadIdx.x == 0) {
        const bool active = !sc->converged && sc->iters < sc->iter_max;
        sc->active = sc->entered = active ? 1u : 0u;
        if (active) {
            sc->iters += 1;
            sc->pap = pap;
            sc->alpha = p_div(sc->rz, pap);
        }
    }
}

// UPDATE: r -= ap*alpha first (gated by "active"); always: partials of r.r and r.(r/d)
template <typename T, bool UPDATE>
__global__ void __launch_bounds__(kBlock)
k_pcg_update(const PcgScalars<T> *__restrict__ sc, T *__restrict__ r, const T *__restrict__ ap, const T *__restrict__ d, uint64_t n,
             T *__restrict__ part_rr, T *__restrict__ part_rz) {
    T alpha = T(0);
    if (UPDATE) {
        if (!sc->active) return;  // block-uniform
        alpha = sc->alpha;
    }
    T s_rr = T(0), s_rz = T(0);
    sweep<T>(n, [&](auto at) {
        auto rv = at.load(r);
        const auto dv = at.load(d);
        if (UPDATE) {
            const auto av = at.load(ap);
#pragma unroll
            for (int e = 0; e < at.width; ++e) rv[e] = p_add(rv[e], -p_mul(av[e], alpha));
            at.store(r, rv);
        }
#pragma unroll
        for (int e = 0; e < at.width; ++e) {
            s_rr = p_add(s_rr, p_mul(rv[e], rv[e]));
            s_rz = p_add(s_rz, p_mul(rv[e], p_div(rv[e], dv[e])));
        }
    });
    block_sums(s_rr, s_rz, part_rr, part_rz);
}

// FIRST: rr, rz of the initial residual.  Else: the stop test on r.r (before beta, linearsolver.rs:52-54), then beta = rz' / rz
template <typename T, bool FIRST>
__global__ void __launch_bounds__(kBlock)
k_pcg_beta(PcgScalars<T> *sc, const T *__restrict__ part_a, const T *__restrict__ part_b, unsigned n_parts) {
    if (!FIRST && !sc->active) return;
    __shared__ T out2[2];
    fold2(part_a, part_b, n_parts, out2);
    if (threadIdx.x == 0) {
        const T rr = out2[0], rz = out2[1];
        sc->rr = rr;
        if (FIRST) {
            sc->rz = rz;
        } else if (sqrt((double)rr) < sc->tol) {
            sc->converged = 1;
            sc->active = 0;
        } else {
            sc->beta = p_div(rz, sc->rz);
            sc->rz = rz;
        }
    }
}

// x += p*alpha (the entered body's update, linearsolver.rs:47 -- carried out here because this sweep reads p anyway), then
// p = p*beta + r/d while the loop goes on.  FIRST: p = r/d.
template <typename T, bool FIRST>
__global__ void __launch_bounds__(kBlock)
k_pcg_p(const PcgScalars<T> *__restrict__ sc, T *__restrict__ p, const T *__restrict__ r, const T *__restrict__ d, T *__restrict__ x, uint64_t n) {
    T alpha = T(0), beta = T(0);
    bool rebuild = true;
    if (!FIRST) {
        if (!sc->entered) return;
        alpha = sc->alpha;
        beta = sc->beta;
        rebuild = sc->active != 0;
    }
    sweep<T>(n, [&](auto at) {
        typename decltype(at)::pack pv;
        if (!FIRST) {
            pv = at.load(p);
            auto xv = at.load(x);
#pragma unroll
            for (int e = 0; e < at.width; ++e) xv[e] = p_add(xv[e], p_mul(pv[e], alpha));
            at.store(x, xv);
        }
        if (rebuild) {
            const auto rv = at.load(r), dv = at.load(d);
#pragma unroll
            for (int e = 0; e < at.width; ++e) {
                const T z = p_div(rv[e], dv[e]);
                pv[e] = FIRST ? z : p_add(p_mul(pv[e], beta), z);
            }
            at.store(p, pv);
        }
    });
}

// ---- host side: what the Jacobi driver here and the launched one below share (the preconditioner's set-up: precond.hpp) ---------------
// Where p.Ap comes from after the product Ap = A p that was handed d_dot: out of the product's epilogue when the kernel offers it
// (K1s: n_dot per-tile partials in d_dot; more than 1024 of them are folded by a full grid first), else a separate two-stage dot.
// Enqueues what that takes and returns what k_pcg_alpha folds.  dot_scratch: 2 * kReducePartials + 8 values (the dot's partials,
// its result, the first fold).
template <typename T>
struct PapSource {
    const T *vals;
    uint32_t count;
};
template <typename T>
int pap_source(const T *p, const T *ap, size_t n, const T *d_dot, size_t n_dot, T *dot_scratch, hipStream_t s, PapSource<T> *out) {
    if (d_dot && n_dot > (size_t)kReducePartials) {
        const unsigned fb = reduce_blocks(n_dot);
        T *fold_scratch = dot_scratch + kReducePartials + 8;
        hipLaunchKernelGGL((k_pcg_sum_stage1<T>), dim3(fb), dim3(kBlock), 0, s, d_dot, (uint64_t)n_dot, fold_scratch);
        *out = {fold_scratch, fb};
    } else if (d_dot) {
        *out = {d_dot, (uint32_t)n_dot};
    } else {
        if (n) SMH_TRY(launch_dot(sizeof(T) == 8 ? SMH_F64 : SMH_F32, p, ap, n, dot_scratch, dot_scratch + kReducePartials, s));
        else SMH_HIP(hipMemsetAsync(dot_scratch + kReducePartials, 0, sizeof(T), s));
        *out = {dot_scratch + kReducePartials, 1u};
    }
    return SMH_OK;
}

// (c.b and c.x: host memory; batches of 8, c.check_every is not read)
template <typename T>
int pcg_t(smh_crs *m, const SolveCall &c) {
    const int dt = sizeof(T) == 8 ? SMH_F64 : SMH_F32;
    const size_t n = c.n;
    SolveRun run;
    const unsigned grid = pcg_grid(n);
    return run.run([&]() -> int {
        SMH_TRY(run.own_stream());
        const hipStream_t s = run.s;
        Scratch &ws = run.ws;
        T *d_x = nullptr, *d_r = nullptr, *d_p = nullptr, *d_ap = nullptr, *d_d = nullptr, *d_part = nullptr, *d_dot = nullptr;
        PcgScalars<T> *d_sc = nullptr;
        SMH_TRY(ws.alloc(&d_x, n)); SMH_TRY(ws.alloc(&d_r, n)); SMH_TRY(ws.alloc(&d_p, n));
        SMH_TRY(ws.alloc(&d_ap, n)); SMH_TRY(ws.alloc(&d_d, n));
        SMH_TRY(ws.alloc(&d_part, 2 * (size_t)kPcgBlocks + 2 * (size_t)kReducePartials + 8));
        SMH_TRY(ws.alloc(&d_sc, 1));
        SMH_TRY(precond_setup(jacobi_precond(m), n, d_d, ws, s));
        SMH_TRY(run.h_sc.alloc(sizeof(PcgScalars<T>), hipHostMallocDefault));
        T *part_rr = d_part, *part_rz = d_part + kPcgBlocks, *dot_scratch = d_part + 2 * kPcgBlocks;
        const size_t n_dot = spmv_fused_dot_partials(m, n, c.variant);
        if (n_dot) SMH_TRY(ws.alloc(&d_dot, n_dot));
        // r = b - A x; p = r / d; rr, rz
        hipLaunchKernelGGL((k_pcg_init<T>), dim3(1), dim3(1), 0, s, d_sc, c.tol, (uint64_t)c.iter_max);
        SMH_TRY(stage_residual(m, c.variant, (const T *)c.b, (const T *)c.x, n, d_r, d_x, d_ap, s));
        hipLaunchKernelGGL((k_pcg_update<T, false>), dim3(grid), dim3(kBlock), 0, s, d_sc, d_r, d_ap, d_d, (uint64_t)n, part_rr, part_rz);
        hipLaunchKernelGGL((k_pcg_beta<T, true>), dim3(1), dim3(kBlock), 0, s, d_sc, part_rr, part_rz, grid);
        hipLaunchKernelGGL((k_pcg_p<T, true>), dim3(grid), dim3(kBlock), 0, s, d_sc, d_p, d_r, d_d, d_x, (uint64_t)n);
        SMH_HIP(hipGetLastError());
        // one loop body: SpMV (+ p.Ap), alpha, update of r + partials, stop test / beta, x and p
        auto body = [&]() -> int {
            PapSource<T> pap;
            SMH_TRY(spmv_enqueue(m, d_p, n, d_ap, c.variant, s, d_dot));
            SMH_TRY(pap_source(d_p, d_ap, n, d_dot, n_dot, dot_scratch, s, &pap));
            hipLaunchKernelGGL((k_pcg_alpha<T>), dim3(1), dim3(kBlock), 0, s, d_sc, pap.vals, pap.count);
            hipLaunchKernelGGL((k_pcg_update<T, true>), dim3(grid), dim3(kBlock), 0, s, d_sc, d_r, d_ap, d_d, (uint64_t)n, part_rr, part_rz);
            hipLaunchKernelGGL((k_pcg_beta<T, false>), dim3(1), dim3(kBlock), 0, s, d_sc, part_rr, part_rz, grid);
            hipLaunchKernelGGL((k_pcg_p<T, false>), dim3(grid), dim3(kBlock), 0, s, d_sc, d_p, d_r, d_d, d_x, (uint64_t)n);
            SMH_HIP(hipGetLastError());
            return SMH_OK;
        };
        SMH_TRY(run.loop(dt, c.iter_max, 8, body, d_sc));
        if (n) SMH_HIP(hipMemcpyAsync(c.x, d_x, n * sizeof(T), hipMemcpyDeviceToHost, s));
        SMH_HIP(hipStreamSynchronize(s));
        return SMH_OK;
    }, c.iters_out, c.rr_out);
}


// ---- symmetric Gauss-Seidel: M = (D + L) D^-1 (D + U), z = M^-1 r by two triangular solves (trisolve.hip) ---------------------------
// The recurrence above with that z, which is a vector here: w = (D + L)^-1 r, then z = (D + U)^-1 (w * d) with the product formed
// inside the upper solve.  The sums are Jacobi's (k_pcg_update's sweep and the one-workgroup fold), one at a time; p.Ap as above.

// per-workgroup partials of x.y (with x == y: of r.r), gated by "active" unless ALWAYS
template <typename T, bool ALWAYS>
__global__ void __launch_bounds__(kBlock)
k_sgs_dot(const PcgScalars<T> *__restrict__ sc, const T *__restrict__ x, const T *__restrict__ y, uint64_t n, T *__restrict__ part) {
    if (!ALWAYS && !sc->active) return;
    block_partial(sweep_dot<T, kPlain>(x, y, n), part);
}

// the entered body's r -= ap*alpha and x += p*alpha in one sweep, and the partials of the new r.r
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_sgs_update(const PcgScalars<T> *__restrict__ sc, T *__restrict__ r, const T *__restrict__ ap, const T *__restrict__ p, T *__restrict__ x, uint64_t n,
             T *__restrict__ part_rr) {
    if (!sc->active) return;  // block-uniform
    const T alpha = sc->alpha;
    T s_rr = T(0);
    sweep<T, kBy16Bytes, kPlain>(n, [&](auto at) {
        auto rv = at.load(r), xv = at.load(x);
        const auto av = at.load(ap), pv = at.load(p);
#pragma unroll
        for (int e = 0; e < at.width; ++e) {
            rv[e] = p_add(rv[e], -p_mul(av[e], alpha));
            xv[e] = p_add(xv[e], p_mul(pv[e], alpha));
            s_rr = p_add(s_rr, p_mul(rv[e], rv[e]));
        }
        at.store(r, rv);
        at.store(x, xv);
    });
    block_partial(s_rr, part_rr);
}

// one workgroup folds the partials.  WHAT 0: rr of the initial residual; 1: rr, then the stop test (before beta); 2: the first
// r.z; 3: rz' = r.z, beta = rz' / rz, rz = rz'
template <typename T, int WHAT>
__global__ void __launch_bounds__(kBlock) k_sgs_fold(PcgScalars<T> *sc, const T *__restrict__ part, unsigned n_parts) {
    if ((WHAT == 1 || WHAT == 3) && !sc->active) return;
    const T v = fold1(part, n_parts);
    if (threadIdx.x == 0) {
        if (WHAT == 0) {
            sc->rr = v;
        } else if (WHAT == 1) {
            sc->rr = v;
            if (sqrt((double)v) < sc->tol) {
                sc->converged = 1;
                sc->active = 0;
            }
        } else if (WHAT == 2) {
            sc->rz = v;
        } else {
            sc->beta = p_div(v, sc->rz);
            sc->rz = v;
        }
    }
}

// p = p*beta + z while the loop goes on.  FIRST: p = z
template <typename T, bool FIRST>
__global__ void __launch_bounds__(kBlock) k_sgs_p(const PcgScalars<T> *__restrict__ sc, T *__restrict__ p, const T *__restrict__ z, uint64_t n) {
    if (!FIRST && !sc->active) return;
    const T beta = FIRST ? T(0) : sc->beta;
    sweep<T, kByElement>(n, [&](auto at) {
        auto pv = at.load(z);
        if (!FIRST) {
            const auto old = at.load(p);
#pragma unroll
            for (int e = 0; e < at.width; ++e) pv[e] = p_add(p_mul(old[e], beta), pv[e]);
        }
        at.store(p, pv);
    });
}

// pc: applied by launches (kPcLaunched)
template <typename T>
int pcg_launched_t(smh_crs *m, const Precond &pc, const SolveCall &c) {
    const int dt = sizeof(T) == 8 ? SMH_F64 : SMH_F32;
    const size_t n = c.n;
    SolveRun run;
    const unsigned grid = pcg_grid(n);
    return run.run([&]() -> int {
        SMH_TRY(precond_prepare(pc));
        SMH_TRY(run.own_stream());
        const hipStream_t s = run.s;
        Scratch &ws = run.ws;
        T *d_x = nullptr, *d_r = nullptr, *d_p = nullptr, *d_ap = nullptr, *d_z = nullptr, *d_w = nullptr, *d_part = nullptr, *d_dot = nullptr;
        PcgScalars<T> *d_sc = nullptr;
        SMH_TRY(ws.alloc(&d_x, n)); SMH_TRY(ws.alloc(&d_r, n)); SMH_TRY(ws.alloc(&d_p, n));
        SMH_TRY(ws.alloc(&d_ap, n)); SMH_TRY(ws.alloc(&d_z, n)); SMH_TRY(ws.alloc(&d_w, n));
        SMH_TRY(ws.alloc(&d_part, (size_t)kPcgBlocks + 2 * (size_t)kReducePartials + 8));
        SMH_TRY(ws.alloc(&d_sc, 1));
        SMH_TRY(precond_setup(pc, n, d_w, ws, s));  // (a probed diagonal's values are read once, there: d_w is overwritten later)
        SMH_TRY(run.h_sc.alloc(sizeof(PcgScalars<T>), hipHostMallocDefault));
        T *part = d_part, *dot_scratch = d_part + kPcgBlocks;
        const size_t n_dot = spmv_fused_dot_partials(m, n, c.variant);
        if (n_dot) SMH_TRY(ws.alloc(&d_dot, n_dot));
        const uint32_t *active = &d_sc->active;
        // r = b - A x; z = M^-1 r; rr, rz; p = z
        hipLaunchKernelGGL((k_pcg_init<T>), dim3(1), dim3(1), 0, s, d_sc, c.tol, (uint64_t)c.iter_max);
        SMH_TRY(stage_residual(m, c.variant, (const T *)c.b, (const T *)c.x, n, d_r, d_x, d_ap, s));
        SMH_TRY(precond_apply_enqueue(pc, d_r, d_w, d_z, nullptr, s));
        hipLaunchKernelGGL((k_sgs_dot<T, true>), dim3(grid), dim3(kBlock), 0, s, d_sc, d_r, d_r, (uint64_t)n, part);
        hipLaunchKernelGGL((k_sgs_fold<T, 0>), dim3(1), dim3(kBlock), 0, s, d_sc, part, grid);
        hipLaunchKernelGGL((k_sgs_dot<T, true>), dim3(grid), dim3(kBlock), 0, s, d_sc, d_r, d_z, (uint64_t)n, part);
        hipLaunchKernelGGL((k_sgs_fold<T, 2>), dim3(1), dim3(kBlock), 0, s, d_sc, part, grid);
        hipLaunchKernelGGL((k_sgs_p<T, true>), dim3(grid), dim3(kBlock), 0, s, d_sc, d_p, d_z, (uint64_t)n);
        SMH_HIP(hipGetLastError());
        size_t spmv_nodes = 1;
        auto body = [&]() -> int {
            PapSource<T> pap;
            SMH_TRY(spmv_enqueue(m, d_p, n, d_ap, c.variant, s, d_dot));
            SMH_TRY(pap_source(d_p, d_ap, n, d_dot, n_dot, dot_scratch, s, &pap));
            hipLaunchKernelGGL((k_pcg_alpha<T>), dim3(1), dim3(kBlock), 0, s, d_sc, pap.vals, pap.count);
            hipLaunchKernelGGL((k_sgs_update<T>), dim3(grid), dim3(kBlock), 0, s, d_sc, d_r, d_ap, d_p, d_x, (uint64_t)n, part);
            hipLaunchKernelGGL((k_sgs_fold<T, 1>), dim3(1), dim3(kBlock), 0, s, d_sc, part, grid);
            SMH_TRY(precond_apply_enqueue(pc, d_r, d_w, d_z, active, s));
            hipLaunchKernelGGL((k_sgs_dot<T, false>), dim3(grid), dim3(kBlock), 0, s, d_sc, d_r, d_z, (uint64_t)n, part);
            hipLaunchKernelGGL((k_sgs_fold<T, 3>), dim3(1), dim3(kBlock), 0, s, d_sc, part, grid);
            hipLaunchKernelGGL((k_sgs_p<T, false>), dim3(grid), dim3(kBlock), 0, s, d_sc, d_p, d_z, (uint64_t)n);
            SMH_HIP(hipGetLastError());
            return SMH_OK;
        };
        // the node budget of a captured batch: the application's launches, the product (a few nodes at most) and the tail of 8
        bool capture = true;
        const size_t bodies = bodies_within_budget(precond_apply_nodes(pc) + spmv_nodes + 3 + 8, c.check_every, &capture);
        SMH_TRY(run.loop(dt, c.iter_max, bodies, body, d_sc, capture));
        if (n) SMH_HIP(hipMemcpyAsync(c.x, d_x, n * sizeof(T), hipMemcpyDefault, s));
        SMH_HIP(hipStreamSynchronize(s));
        return SMH_OK;
    }, c.iters_out, c.rr_out);
}

// the handles' check, then the driver of the matrix's dtype
int pcg_launched(smh_crs *m, const Precond &pc, const SolveCall &c) {
    SMH_TRY(precond_check_handles(pc));
    return m->dtype == SMH_F64 ? pcg_launched_t<double>(m, pc, c) : pcg_launched_t<float>(m, pc, c);
}

}  // namespace

// The entry points: the statuses are decided here (check_solve_vec / check_solve_host, solver_host.hpp), before any launch.
// check_every = 0, and the host forms, stand for 8 bodies per poll.
constexpr size_t kPcgCheckEvery = 8;

extern "C" int smh_pcg_jacobi_solve(smh_crs *m, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len, double tol,
                                    size_t iter_max, int variant, size_t *iters_out, double *rr_out) {
    SMH_TRY(check_solve_host(m, b_host, b_len, x_host_inout, x_len, /*null_vectors*/ true, /*refuse_aliased*/ false));
    const SolveCall c{b_host, x_host_inout, m->n_rows, tol, iter_max, variant, kPcgCheckEvery, iters_out, rr_out};
    return m->dtype == SMH_F64 ? pcg_t<double>(m, c) : pcg_t<float>(m, c);
}

// ---- the symmetric Gauss-Seidel preconditioner and its CG -----------------------------------------------------------------------------
extern "C" int smh_crs_sgs_apply_vec(smh_crs *m, const smh_vec *r, smh_vec *z) {
    if (!m || !r || !z) return fail(SMH_ERR_INVALID, "NULL handle");
    return precond_apply_vec(sgs_precond(m), r, z, "sgs_apply");
}

extern "C" int smh_pcg_sgs_solve_vec(smh_crs *m, const smh_vec *b, smh_vec *x, double tol, size_t iter_max, int variant, size_t check_every,
                                     size_t *iters_out, double *rr_out) {
    SMH_TRY(check_solve_vec(m, b, x, kVecDtype, /*refuse_aliased*/ true, &check_every, kPcgCheckEvery));
    return pcg_launched(m, sgs_precond(m), {b->d, x->d, m->n_rows, tol, iter_max, variant, check_every, iters_out, rr_out});
}

extern "C" int smh_pcg_sgs_solve(smh_crs *m, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len, double tol, size_t iter_max,
                                 int variant, size_t *iters_out, double *rr_out) {
    SMH_TRY(check_solve_host(m, b_host, b_len, x_host_inout, x_len, /*null_vectors*/ true, /*refuse_aliased*/ false));
    return pcg_launched(m, sgs_precond(m), {b_host, x_host_inout, m->n_rows, tol, iter_max, variant, kPcgCheckEvery, iters_out, rr_out});
}

// ---- ILU(0): the same recurrence and application with the solves on a factor handle (smh_crs_ilu0, ilu.hip); the product and its
// fused p.Ap come from a ----------------------------------------------------------------------------------------------------------
extern "C" int smh_crs_ilu_apply_vec(smh_crs *f, const smh_vec *r, smh_vec *z) {
    if (!f || !r || !z) return fail(SMH_ERR_INVALID, "NULL handle");
    return precond_apply_vec(ilu_precond(f), r, z, "ilu_apply");
}

extern "C" int smh_pcg_ilu_solve_vec(smh_crs *a, smh_crs *f, const smh_vec *b, smh_vec *x, double tol, size_t iter_max, int variant, size_t check_every,
                                     size_t *iters_out, double *rr_out) {
    if (!f) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(check_solve_vec(a, b, x, kVecDtype, /*refuse_aliased*/ true, &check_every, kPcgCheckEvery, f));
    return pcg_launched(a, ilu_precond(f), {b->d, x->d, a->n_rows, tol, iter_max, variant, check_every, iters_out, rr_out});
}

extern "C" int smh_pcg_ilu_solve(smh_crs *a, smh_crs *f, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len, double tol, size_t iter_max,
                                 int variant, size_t *iters_out, double *rr_out) {
    if (!f) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(check_solve_host(a, b_host, b_len, x_host_inout, x_len, /*null_vectors*/ true, /*refuse_aliased*/ false, f));
    return pcg_launched(a, ilu_precond(f), {b_host, x_host_inout, a->n_rows, tol, iter_max, variant, kPcgCheckEvery, iters_out, rr_out});
}

// ---- FSAI: the same recurrence with z = G^T (G r) by two products on the factor handles (smh_crs_fsai, fsai.hip), each through its
// own AUTO kernel; variant is a's product's ----------------------------------------------------------------------------------------

extern "C" int smh_crs_fsai_apply_vec(smh_crs *g, smh_crs *gt, const smh_vec *r, smh_vec *z) {
    if (!g || !gt || !r || !z) return fail(SMH_ERR_INVALID, "NULL handle");
    return precond_apply_vec(fsai_precond(g, gt), r, z, "fsai_apply");
}

// the name the documents of the non-symmetric pair (G_L, G_U) use: w = G_L r, z = G_U w
extern "C" int smh_crs_fsai_ns_apply_vec(smh_crs *gl, smh_crs *gu, const smh_vec *r, smh_vec *z) { return smh_crs_fsai_apply_vec(gl, gu, r, z); }

extern "C" int smh_pcg_fsai_solve_vec(smh_crs *a, smh_crs *g, smh_crs *gt, const smh_vec *b, smh_vec *x, double tol, size_t iter_max, int variant,
                                      size_t check_every, size_t *iters_out, double *rr_out) {
    SMH_TRY(check_pair_vec(a, g, gt, kFsaiName, b, x, &check_every, kPcgCheckEvery));
    return pcg_launched(a, fsai_precond(g, gt), {b->d, x->d, a->n_rows, tol, iter_max, variant, check_every, iters_out, rr_out});
}

extern "C" int smh_pcg_fsai_solve(smh_crs *a, smh_crs *g, smh_crs *gt, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len, double tol,
                                  size_t iter_max, int variant, size_t *iters_out, double *rr_out) {
    SMH_TRY(check_pair_host(a, g, gt, kFsaiName, b_host, b_len, x_host_inout, x_len, /*refuse_aliased*/ false));
    return pcg_launched(a, fsai_precond(g, gt), {b_host, x_host_inout, a->n_rows, tol, iter_max, variant, kPcgCheckEvery, iters_out, rr_out});
}
