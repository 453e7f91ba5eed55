// bicgstab.hip -- BiCGSTAB (van der Vorst, unpreconditioned) for non-symmetric systems, gfx950.
//
// An EXTENSION: the reference's only solver is ConjugateGradient (linearsolver.rs:12-61), which needs a symmetric positive
// definite matrix.  This is the stabilised bi-conjugate gradient recurrence in the family's conventions -- the guards of
// linearsolver.rs:30-36, the stop rule sqrt(f64(r.r)) < tol tested before beta (:52-54), no stop test before the first body,
// one rounding per operation (a - b*c is add(a, -mul(b, c)); nothing is contracted), products by the matrix's own kernel:
//   r = b - A x;  r^ = r;  p = r;  rho = r^.r;  rr = r.r
//   body:  v = A p;  rv = r^.v;                  rv == 0: breakdown 2, stop (x untouched by this body)
//          alpha = rho / rv;  s = r - v*alpha;  ss = s.s
//                                                sqrt(f64(ss)) < tol: x += p*alpha; rr = ss; converged ("half-step stop")
//          t = A s;  ts = t.s;  tt = t.t;        tt == 0: x += p*alpha; rr = ss; breakdown 3, stop
//          omega = ts / tt;  x = (x + p*alpha) + s*omega;  r = s - t*omega;  rr = r.r;  rho' = r^.r
//                                                sqrt(f64(rr)) < tol: converged
//                                                rho' == 0 or omega == 0: breakdown 1, stop (x keeps this body's update)
//          beta = (rho'/rho) * (alpha/omega);  rho = rho';  p = r + (p - v*omega)*beta
// The comparisons with zero are exact and NaN compares false, so non-finite data run to iter_max as they do in CG.
//
// Kernels: beside the two products a body is five sweeps -- partials of r^.v (2 n values); s and partials of s.s (3 n);
// partials of t.s and t.t (2 n); x, r and partials of r.r and r^.r (7 n); p (4 n): 18 n values -- each followed (but the
// last) by a one-workgroup kernel that folds the partials, takes the stage's decision and advances the scalars.  All scalars
// live in device memory: a leading block in CgScalars' layout, which solve_in_batches (internal.hpp) polls once
// per batch and whose `converged` word means STOPPED (a breakdown too), and a second block (rho, the dots, omega, the
// breakdown code) that the host reads once after the loop.  Gate words: `active` (this body runs; dropped by the stage that
// stops) gates every sweep after alpha; `xmode` tells the x / r sweep what is due (0 nothing, 1 x += p*alpha alone, 2 all).
// Bodies enqueued past the stop are no-ops, so x, rr, iters and the code are the stopping body's wherever it falls in a batch.
// Sweeps and reductions: solver_tree.hpp's everywhere -- its sweep, its workgroup sums, fold1 / fold2 over the partials --
// deterministic, no float atomics.  One stream, one linear chain of launches.
//
// Right-preconditioned (smh_bicgstab_precond_solve*): A M^-1 u = b, x = M^-1 u, so the residual the recurrence carries is the true
// one and the stop rule, rr, iters and the three codes keep their meaning.  What changes in the recurrence above:
//   set-up:  nothing (M is not applied to the residual)
//   body:    p^ = M^-1 p;  v = A p^;   ...   s^ = M^-1 s;  t = A s^;   x takes p^*alpha and s^*omega (r, the dots and p as above)
// x does not feed back, so from x0 = 0 every scalar is the unpreconditioned recurrence's on the product A o M^-1.
// The driver and the kernels that differ are instantiated per PrecondShape (precond.hpp); kPcNone's chain of launches is the one
// described above, launch for launch.
// kPcFused (Jacobi): M^-1 v is v_i / d_i, a division, d_i the first stored (i, i) (precond.hpp's probe), and costs no launch in a body: the p
// sweep writes p and p^ = p / d (4 n -> 6 n), the s sweep s and s^ = s / d (3 n -> 5 n), the x / r sweep reads p^ and s^ for x and s for
// r (7 n -> 8 n; dividing p and s again in registers would read d for one of them: the same 8 n, and two divisions more) -- 23 n
// values beside the two products, against 18 n.  The set-up forms p^ = r / d in one sweep of its own.  Ten vectors of storage.
// kPcLaunched: M^-1 is applied by launches of its own (Precond, precond.hpp); for SGS on the matrix itself and ILU(0) on a factor,
// two level-scheduled triangular solves on one handle.  The body opens with the application p -> p^ and the s application s -> s^ follows the half-step stage; the products read
// p^ and s^; the sweeps are kPcNone's but for the x / r sweep (8 n).  Every triangular launch takes a device gate word: the s
// application `active`, the p application BiMore::enter -- "the next body will be entered" -- which the set-up leaves (iter_max == 0
// closes it), every stage that stops and a body that is not entered clear, and the beta stage sets (iters == iter_max is a stop
// there); so bodies enqueued past the stop run no solve.  Ten vectors of storage (p^, s^, the solves' scratch).  A captured batch
// holds two applications per body: bodies_within_budget (precond.hpp) makes the batches smaller or drops the capture, which changes
// no bit.
// A pair of product handles (smh_bicgstab_fsai_solve*: M^-1 v = gt (g v), fsai.hip's factors) runs the same chain with Precond's products and
// the same ten vectors.  Both applications are two products through the handles' own AUTO kernels, ungated as the body's own products
// are: past the stop they form the same p^ and s^ from unchanged p and s again, and every sweep that writes x, r or p stays gated.
// Host side: the driver (bicgstab_t) is its allocations, its set-up launches, the body lambda and SolveRun::run (solver_host.hpp:
// the stream of its own, the workspaces, the drain, r = b - A x); the entry points' argument checks are solver_host.hpp's.
#include "internal.hpp"
#include "precond.hpp"
#include "solver_host.hpp"
#include "solver_tree.hpp"

#include <cmath>

using namespace smh;

namespace {

// ---- device-resident scalars ---------------------------------------------------------------------------------------------
// the block the host polls through CG's reader (cg_read_scalars): rr, the stop word and the body count sit where CG's do
template <typename T>
struct BiScalars {
    T rr, alpha, beta, spare0_, spare1_;
    uint32_t converged;  // STOPPED: converged, or a breakdown
    uint32_t active;     // this body runs (not stopped, fewer than iter_max bodies entered, no stage of it has stopped yet)
    uint32_t xmode;      // what this body's x / r sweep does: 0 nothing, 1 x += p*alpha, 2 x, r and the partials
    uint32_t pad_;
    uint64_t iters;
    uint64_t iter_max;
    double tol;
};
static_assert(scalars_like_cg<BiScalars>(), "BiScalars and CgScalars have drifted apart");
// the solver's further scalars: read by the host once, after the loop
template <typename T>
struct BiMore {
    T rho, rv, ss, ts, tt, omega;
    uint32_t breakdown;  // 0 none, 1 rho' == 0 or omega == 0, 2 r^.v == 0, 3 t.t == 0 (a stop with code 0 was a stop test's)
    uint32_t enter;      // gate: the next body will be entered (kPcLaunched's application p -> p^ that opens it is due)
};

template <typename T>
__global__ void k_bi_init(BiScalars<T> *sc, BiMore<T> *mo, double tol, uint64_t iter_max) {
    sc->rr = sc->alpha = sc->beta = sc->spare0_ = sc->spare1_ = T(0);
    sc->converged = sc->active = sc->xmode = sc->pad_ = 0;
    sc->iters = 0;
    sc->iter_max = iter_max;
    sc->tol = tol;
    mo->rho = mo->rv = mo->ss = mo->ts = mo->tt = mo->omega = T(0);
    mo->breakdown = mo->enter = 0;
}

// ---- the sweeps (solver_tree.hpp's sweep: the workspaces are pool allocations, aligned) ---------------------------------------------
// partials of a.b (r^.v): runs when the body that follows will be entered
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_bi_dot(const BiScalars<T> *__restrict__ sc, const T *__restrict__ a, const T *__restrict__ b, uint64_t n, T *__restrict__ part) {
    if (sc->converged || sc->iters >= sc->iter_max) return;  // block-uniform
    block_partial(sweep_dot(a, b, n), part);
}

// partials of t.s and t.t in one sweep.  SETUP (t = s = r): the initial rho = r^.r and r.r, ungated
template <typename T, bool SETUP>
__global__ void __launch_bounds__(kBlock)
k_bi_dot2(const BiScalars<T> *__restrict__ sc, const T *__restrict__ t, const T *__restrict__ s, uint64_t n, T *__restrict__ part_ts,
          T *__restrict__ part_tt) {
    if (!SETUP && !sc->active) return;
    T a_ts = T(0), a_tt = T(0);
    sweep<T>(n, [&](auto at) {
        const auto tv = at.load(t), sv = at.load(s);
#pragma unroll
        for (int e = 0; e < at.width; ++e) {
            a_ts = p_add(a_ts, p_mul(tv[e], sv[e]));
            a_tt = p_add(a_tt, p_mul(tv[e], tv[e]));
        }
    });
    block_sums(a_ts, a_tt, part_ts, part_tt);
}

// s = r - v*alpha; partials of s.s.  kPcFused: and s^ = s / diag, the second product's input
template <typename T, PrecondShape P = kPcNone>
__global__ void __launch_bounds__(kBlock)
k_bi_s(const BiScalars<T> *__restrict__ sc, const T *__restrict__ r, const T *__restrict__ v, T *__restrict__ s, uint64_t n, T *__restrict__ part_ss,
       const T *__restrict__ diag = nullptr, T *__restrict__ shat = nullptr) {
    if (!sc->active) return;
    const T alpha = sc->alpha;
    T acc = T(0);
    sweep<T>(n, [&](auto at) {
        auto sv = at.load(r);
        const auto vv = at.load(v);
#pragma unroll
        for (int e = 0; e < at.width; ++e) {
            sv[e] = p_add(sv[e], -p_mul(vv[e], alpha));
            acc = p_add(acc, p_mul(sv[e], sv[e]));
        }
        at.store(s, sv);
        if constexpr (P == kPcFused) {
            const auto dv = at.load(diag);
#pragma unroll
            for (int e = 0; e < at.width; ++e) sv[e] = p_div(sv[e], dv[e]);
            at.store(shat, sv);
        }
    });
    block_partial(acc, part_ss);
}

// xmode 2: x = (x + p*alpha) + s*omega; r = s - t*omega; partials of r.r and r^.r.  xmode 1 (half-step stop, breakdown 3): x += p*alpha.
// PRE (preconditioned): p is p^ in both modes and x takes shat = s^ where r takes s
template <typename T, bool PRE = false>
__global__ void __launch_bounds__(kBlock)
k_bi_xr(const BiScalars<T> *__restrict__ sc, const BiMore<T> *__restrict__ mo, T *__restrict__ x, const T *__restrict__ p, const T *__restrict__ s,
        const T *__restrict__ t, const T *__restrict__ rhat, T *__restrict__ r, uint64_t n, T *__restrict__ part_rr, T *__restrict__ part_rho,
        const T *__restrict__ shat = nullptr) {
    const uint32_t mode = sc->xmode;  // block-uniform
    if (mode == 0) return;
    const T alpha = sc->alpha;
    if (mode == 1) {
        sweep<T>(n, [&](auto at) {
            auto xv = at.load(x);
            const auto pv = at.load(p);
#pragma unroll
            for (int e = 0; e < at.width; ++e) xv[e] = p_add(xv[e], p_mul(pv[e], alpha));
            at.store(x, xv);
        });
        return;
    }
    const T omega = mo->omega;
    T a_rr = T(0), a_rho = T(0);
    sweep<T>(n, [&](auto at) {
        auto xv = at.load(x);
        const auto pv = at.load(p), sv = at.load(s), tv = at.load(t), hv = at.load(rhat);
        typename decltype(at)::pack rv, qv;  // qv: what x takes beside p (s, or s^)
        if constexpr (PRE) qv = at.load(shat);
        else qv = sv;
#pragma unroll
        for (int e = 0; e < at.width; ++e) {
            xv[e] = p_add(p_add(xv[e], p_mul(pv[e], alpha)), p_mul(qv[e], omega));
            rv[e] = p_add(sv[e], -p_mul(tv[e], omega));
            a_rr = p_add(a_rr, p_mul(rv[e], rv[e]));
            a_rho = p_add(a_rho, p_mul(hv[e], rv[e]));
        }
        at.store(x, xv);
        at.store(r, rv);
    });
    block_sums(a_rr, a_rho, part_rr, part_rho);
}

// p = r + (p - v*omega)*beta.  kPcFused: and p^ = p / diag, the first product's input
template <typename T, PrecondShape P = kPcNone>
__global__ void __launch_bounds__(kBlock)
k_bi_p(const BiScalars<T> *__restrict__ sc, const BiMore<T> *__restrict__ mo, T *__restrict__ p, const T *__restrict__ r, const T *__restrict__ v, uint64_t n,
       const T *__restrict__ diag = nullptr, T *__restrict__ phat = nullptr) {
    if (!sc->active) return;
    const T beta = sc->beta, omega = mo->omega;
    sweep<T>(n, [&](auto at) {
        auto pv = at.load(p);
        const auto rv = at.load(r), vv = at.load(v);
#pragma unroll
        for (int e = 0; e < at.width; ++e) pv[e] = p_add(rv[e], p_mul(p_add(pv[e], -p_mul(vv[e], omega)), beta));
        at.store(p, pv);
        if constexpr (P == kPcFused) {
            const auto dv = at.load(diag);
#pragma unroll
            for (int e = 0; e < at.width; ++e) pv[e] = p_div(pv[e], dv[e]);
            at.store(phat, pv);
        }
    });
}

// kPcFused's set-up: p^ = p / diag (p = r)
template <typename T>
__global__ void __launch_bounds__(kBlock) k_bi_phat0(const T *__restrict__ p, const T *__restrict__ diag, T *__restrict__ phat, uint64_t n) {
    sweep<T>(n, [&](auto at) {
        auto pv = at.load(p);
        const auto dv = at.load(diag);
#pragma unroll
        for (int e = 0; e < at.width; ++e) pv[e] = p_div(pv[e], dv[e]);
        at.store(phat, pv);
    });
}

// ---- the one-workgroup kernels between the sweeps -----------------------------------------------------------------------
// rho = r^.r and rr = r.r of the initial residual
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_bi_setup(BiScalars<T> *sc, BiMore<T> *mo, const T *__restrict__ part_rho, const T *__restrict__ part_rr, unsigned n_parts) {
    __shared__ T out2[2];
    fold2(part_rho, part_rr, n_parts, out2);
    if (threadIdx.x == 0) {
        mo->rho = out2[0];
        sc->rr = out2[1];
        mo->enter = sc->iter_max ? 1u : 0u;
    }
}

// decide whether this body runs; rv = r^.v; rv == 0: breakdown 2; else alpha = rho / rv
template <typename T>
__global__ void __launch_bounds__(kBlock) k_bi_alpha(BiScalars<T> *sc, BiMore<T> *mo, const T *__restrict__ part, unsigned n_parts) {
    const bool active = !sc->converged && sc->iters < sc->iter_max;  // (every thread reads before thread 0 writes: the fold has a barrier)
    if (!active) {
        if (threadIdx.x == 0) sc->active = sc->xmode = mo->enter = 0;
        return;
    }
    const T rv = fold1(part, n_parts);
    if (threadIdx.x == 0) {
        sc->iters += 1;
        sc->xmode = 0;
        mo->rv = rv;
        if (rv == T(0)) {
            mo->breakdown = 2;
            sc->converged = 1;
            sc->active = mo->enter = 0;
        } else {
            sc->active = 1;
            sc->alpha = p_div(mo->rho, rv);
        }
    }
}

// ss = s.s; the half-step stop
template <typename T>
__global__ void __launch_bounds__(kBlock) k_bi_half(BiScalars<T> *sc, BiMore<T> *mo, const T *__restrict__ part, unsigned n_parts) {
    if (!sc->active) return;
    const T ss = fold1(part, n_parts);
    if (threadIdx.x == 0) {
        mo->ss = ss;
        if (sqrt((double)ss) < sc->tol) {
            sc->rr = ss;
            sc->xmode = 1;
            sc->converged = 1;
            sc->active = mo->enter = 0;
        }
    }
}

// ts = t.s, tt = t.t; tt == 0: breakdown 3; else omega = ts / tt
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_bi_omega(BiScalars<T> *sc, BiMore<T> *mo, const T *__restrict__ part_ts, const T *__restrict__ part_tt, unsigned n_parts) {
    if (!sc->active) return;
    __shared__ T out2[2];
    fold2(part_ts, part_tt, n_parts, out2);
    if (threadIdx.x == 0) {
        const T ts = out2[0], tt = out2[1];
        mo->ts = ts;
        mo->tt = tt;
        if (tt == T(0)) {
            sc->rr = mo->ss;
            sc->xmode = 1;
            mo->breakdown = 3;
            sc->converged = 1;
            sc->active = mo->enter = 0;
        } else {
            mo->omega = p_div(ts, tt);
            sc->xmode = 2;
        }
    }
}

// rr = r.r, rho' = r^.r; the stop test (before beta, linearsolver.rs:52-54); rho' == 0 or omega == 0: breakdown 1; else beta, rho = rho'
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_bi_beta(BiScalars<T> *sc, BiMore<T> *mo, const T *__restrict__ part_rr, const T *__restrict__ part_rho, unsigned n_parts) {
    if (!sc->active) return;
    __shared__ T out2[2];
    fold2(part_rr, part_rho, n_parts, out2);
    if (threadIdx.x == 0) {
        const T rr = out2[0], rho_new = out2[1], omega = mo->omega;
        sc->rr = rr;
        if (sqrt((double)rr) < sc->tol) {
            sc->converged = 1;
            sc->active = mo->enter = 0;
        } else if (rho_new == T(0) || omega == T(0)) {
            mo->breakdown = 1;
            sc->converged = 1;
            sc->active = mo->enter = 0;
        } else {
            sc->beta = p_mul(p_div(rho_new, mo->rho), p_div(sc->alpha, omega));
            mo->rho = rho_new;
            mo->enter = sc->iters < sc->iter_max ? 1u : 0u;  // (iters == iter_max is a stop)
        }
    }
}

// P: precond_shape(pc).  kPcNone's chain of launches is the unpreconditioned solver's, launch for launch.
template <typename T, PrecondShape P>
int bicgstab_t(smh_crs *m, const Precond &pc, const SolveCall &c) {
    const int dt = sizeof(T) == 8 ? SMH_F64 : SMH_F32;
    const size_t n = c.n;
    constexpr bool PRE = P != kPcNone;
    SolveRun run;  // (its `converged` means STOPPED here)
    int breakdown = 0;
    const unsigned grid = pcg_grid(n);
    const int rc = run.run([&]() -> int {
        SMH_TRY(precond_prepare(pc));
        SMH_TRY(run.own_stream());
        const hipStream_t s = run.s;
        Scratch &ws = run.ws;
        T *x = nullptr, *r = nullptr, *rhat = nullptr, *p = nullptr, *v = nullptr, *sv = nullptr, *t = nullptr, *part = nullptr;
        T *phat = nullptr, *shat = nullptr, *diag = nullptr, *tw = nullptr;  // p^ and s^; fused: the diagonal.  Launched: the application's scratch
        BiScalars<T> *sc = nullptr;
        BiMore<T> *mo = nullptr;
        SMH_TRY(ws.alloc(&x, n)); SMH_TRY(ws.alloc(&r, n)); SMH_TRY(ws.alloc(&rhat, n)); SMH_TRY(ws.alloc(&p, n));
        SMH_TRY(ws.alloc(&v, n)); SMH_TRY(ws.alloc(&sv, n)); SMH_TRY(ws.alloc(&t, n));
        SMH_TRY(ws.alloc(&part, 2 * (size_t)kPcgBlocks));
        SMH_TRY(ws.alloc(&sc, 1));
        SMH_TRY(ws.alloc(&mo, 1));
        SMH_TRY(run.h_sc.alloc(sizeof(BiScalars<T>) + sizeof(BiMore<T>), hipHostMallocDefault));
        if constexpr (PRE) { SMH_TRY(ws.alloc(&phat, n)); SMH_TRY(ws.alloc(&shat, n)); }
        if constexpr (P == kPcFused) SMH_TRY(ws.alloc(&diag, n));
        if constexpr (P == kPcLaunched) SMH_TRY(ws.alloc(&tw, n));
        SMH_TRY(precond_setup(pc, n, P == kPcFused ? diag : tw, ws, s));  // (tw: the solves' probe keeps no values)
        T *part_a = part, *part_b = part + kPcgBlocks;
        // r = b - A x; r^ = r; p = r; rho = r^.r; rr = r.r
        hipLaunchKernelGGL((k_bi_init<T>), dim3(1), dim3(1), 0, s, sc, mo, c.tol, (uint64_t)c.iter_max);
        SMH_TRY(stage_residual(m, c.variant, (const T *)c.b, (const T *)c.x, n, r, x, v, s));
        if (n) {
            SMH_HIP(hipMemcpyAsync(rhat, r, n * sizeof(T), hipMemcpyDeviceToDevice, s));
            SMH_HIP(hipMemcpyAsync(p, r, n * sizeof(T), hipMemcpyDeviceToDevice, s));
        }
        hipLaunchKernelGGL((k_bi_dot2<T, true>), dim3(grid), dim3(kBlock), 0, s, sc, r, r, (uint64_t)n, part_a, part_b);
        hipLaunchKernelGGL((k_bi_setup<T>), dim3(1), dim3(kBlock), 0, s, sc, mo, part_a, part_b, grid);
        if constexpr (P == kPcFused) hipLaunchKernelGGL((k_bi_phat0<T>), dim3(grid), dim3(kBlock), 0, s, p, diag, phat, (uint64_t)n);
        SMH_HIP(hipGetLastError());
        const T *pin = PRE ? phat : p, *sin = PRE ? shat : sv;  // what the two products read
        auto body = [&]() -> int {
            if constexpr (P == kPcLaunched) SMH_TRY(precond_apply_enqueue(pc, p, tw, phat, &mo->enter, s));
            SMH_TRY(spmv_enqueue(m, pin, n, v, c.variant, s));
            hipLaunchKernelGGL((k_bi_dot<T>), dim3(grid), dim3(kBlock), 0, s, sc, rhat, v, (uint64_t)n, part_a);
            hipLaunchKernelGGL((k_bi_alpha<T>), dim3(1), dim3(kBlock), 0, s, sc, mo, part_a, grid);
            hipLaunchKernelGGL((k_bi_s<T, P>), dim3(grid), dim3(kBlock), 0, s, sc, r, v, sv, (uint64_t)n, part_a, diag, shat);
            hipLaunchKernelGGL((k_bi_half<T>), dim3(1), dim3(kBlock), 0, s, sc, mo, part_a, grid);
            SMH_HIP(hipGetLastError());
            if constexpr (P == kPcLaunched) SMH_TRY(precond_apply_enqueue(pc, sv, tw, shat, &sc->active, s));
            SMH_TRY(spmv_enqueue(m, sin, n, t, c.variant, s));
            hipLaunchKernelGGL((k_bi_dot2<T, false>), dim3(grid), dim3(kBlock), 0, s, sc, t, sv, (uint64_t)n, part_a, part_b);
            hipLaunchKernelGGL((k_bi_omega<T>), dim3(1), dim3(kBlock), 0, s, sc, mo, part_a, part_b, grid);
            hipLaunchKernelGGL((k_bi_xr<T, PRE>), dim3(grid), dim3(kBlock), 0, s, sc, mo, x, pin, sv, t, rhat, r, (uint64_t)n, part_a, part_b, shat);
            hipLaunchKernelGGL((k_bi_beta<T>), dim3(1), dim3(kBlock), 0, s, sc, mo, part_a, part_b, grid);
            hipLaunchKernelGGL((k_bi_p<T, P>), dim3(grid), dim3(kBlock), 0, s, sc, mo, p, r, v, (uint64_t)n, diag, phat);
            SMH_HIP(hipGetLastError());
            return SMH_OK;
        };
        if constexpr (P == kPcLaunched) {
            // the node budget of a captured batch: two applications, two products (a few nodes each at most) and the chain of 9
            bool capture = true;
            const size_t bodies = bodies_within_budget(2 * precond_apply_nodes(pc) + 2 * (1 + 3) + 9, c.check_every, &capture);
            SMH_TRY(run.loop(dt, c.iter_max, bodies, body, sc, capture));
        } else {
            SMH_TRY(run.loop(dt, c.iter_max, c.check_every, body, sc));
        }
        BiMore<T> *h_mo = (BiMore<T> *)((char *)run.h_sc.get() + sizeof(BiScalars<T>));
        SMH_HIP(hipMemcpyAsync(h_mo, mo, sizeof(BiMore<T>), hipMemcpyDeviceToHost, s));
        if (n) SMH_HIP(hipMemcpyAsync(c.x, x, n * sizeof(T), hipMemcpyDefault, s));
        SMH_HIP(hipStreamSynchronize(s));
        breakdown = (int)h_mo->breakdown;
        return SMH_OK;
    }, c.iters_out, c.rr_out);
    if (rc == SMH_OK && c.breakdown_out) *c.breakdown_out = breakdown;
    return rc;
}

// the handles' check, then the driver of the matrix's dtype and the preconditioner's shape
int bicgstab(smh_crs *m, const Precond &pc, const SolveCall &c) {
    SMH_TRY(precond_check_handles(pc));
    return with_dtype_and_shape(m->dtype, precond_shape(pc), [&](auto t, auto shape) { return bicgstab_t<decltype(t), decltype(shape)::value>(m, pc, c); });
}

constexpr size_t kBiCheckEvery = 8;  // bodies per poll that check_every = 0, and the host form, stand for

}  // namespace

// the statuses are decided here (check_solve_vec / check_solve_host, solver_host.hpp), before any launch
extern "C" int smh_bicgstab_solve_vec(smh_crs *m, const smh_vec *b, smh_vec *x, double tol, size_t iter_max, int variant, size_t check_every,
                                      size_t *iters_out, double *rr_out, int *breakdown_out) {
    SMH_TRY(check_solve_vec(m, b, x, kVecDtype, /*refuse_aliased*/ true, &check_every, kBiCheckEvery));
    return bicgstab(m, no_precond(), {b->d, x->d, m->n_rows, tol, iter_max, variant, check_every, iters_out, rr_out, breakdown_out});
}

extern "C" int smh_bicgstab_solve(smh_crs *m, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len, double tol, size_t iter_max,
                                  int variant, size_t *iters_out, double *rr_out, int *breakdown_out) {
    SMH_TRY(check_solve_host(m, b_host, b_len, x_host_inout, x_len, /*null_vectors*/ true, /*refuse_aliased*/ true));
    return bicgstab(m, no_precond(), {b_host, x_host_inout, m->n_rows, tol, iter_max, variant, kBiCheckEvery, iters_out, rr_out, breakdown_out});
}

// Right-preconditioned: `precond` and `f` first (check_precond, precond.hpp: as smh_gmres_precond_solve*), then the checks above (with
// ILU's factor against the matrix, as smh_pcg_ilu_solve); what needs the device -- a stored column >= n, a zero or absent diagonal
// entry -- is decided in the driver before its first launch
extern "C" int smh_bicgstab_precond_solve_vec(smh_crs *a, int precond, smh_crs *f, const smh_vec *b, smh_vec *x, double tol, size_t iter_max,
                                              int variant, size_t check_every, size_t *iters_out, double *rr_out, int *breakdown_out) {
    SMH_TRY(check_precond(precond, f));
    if (precond == SMH_PRECOND_NONE) return smh_bicgstab_solve_vec(a, b, x, tol, iter_max, variant, check_every, iters_out, rr_out, breakdown_out);
    SMH_TRY(check_solve_vec(a, b, x, kVecDtype, /*refuse_aliased*/ true, &check_every, kBiCheckEvery, f));
    return bicgstab(a, precond_of(precond, a, f), {b->d, x->d, a->n_rows, tol, iter_max, variant, check_every, iters_out, rr_out, breakdown_out});
}

extern "C" int smh_bicgstab_precond_solve(smh_crs *a, int precond, smh_crs *f, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len,
                                          double tol, size_t iter_max, int variant, size_t *iters_out, double *rr_out, int *breakdown_out) {
    SMH_TRY(check_precond(precond, f));
    if (precond == SMH_PRECOND_NONE) return smh_bicgstab_solve(a, b_host, b_len, x_host_inout, x_len, tol, iter_max, variant, iters_out, rr_out, breakdown_out);
    SMH_TRY(check_solve_host(a, b_host, b_len, x_host_inout, x_len, /*null_vectors*/ true, /*refuse_aliased*/ true, f));
    return bicgstab(a, precond_of(precond, a, f), {b_host, x_host_inout, a->n_rows, tol, iter_max, variant, kBiCheckEvery, iters_out, rr_out, breakdown_out});
}

// Right-preconditioned by a pair of product handles, M^-1 v = gt (g v): (G_L, G_U) of smh_crs_fsai_ns, or (G, G^T) of smh_crs_fsai for
// a symmetric a.  The pair's checks are smh_pcg_fsai_solve's; nothing is probed (no operation divides by a factor's value); a stored
// column >= n is decided in the driver before its first launch
extern "C" int smh_bicgstab_fsai_solve_vec(smh_crs *a, smh_crs *g, smh_crs *gt, const smh_vec *b, smh_vec *x, double tol, size_t iter_max, int variant,
                                           size_t check_every, size_t *iters_out, double *rr_out, int *breakdown_out) {
    SMH_TRY(check_pair_vec(a, g, gt, kFsaiName, b, x, &check_every, kBiCheckEvery));
    return bicgstab(a, fsai_precond(g, gt), {b->d, x->d, a->n_rows, tol, iter_max, variant, check_every, iters_out, rr_out, breakdown_out});
}

extern "C" int smh_bicgstab_fsai_solve(smh_crs *a, smh_crs *g, smh_crs *gt, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len, double tol,
                                       size_t iter_max, int variant, size_t *iters_out, double *rr_out, int *breakdown_out) {
    SMH_TRY(check_pair_host(a, g, gt, kFsaiName, b_host, b_len, x_host_inout, x_len, /*refuse_aliased*/ true));
    return bicgstab(a, fsai_precond(g, gt), {b_host, x_host_inout, a->n_rows, tol, iter_max, variant, kBiCheckEvery, iters_out, rr_out, breakdown_out});
}
