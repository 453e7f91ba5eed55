// gmres.hip -- restarted GMRES(m) (Saad & Schultz), unpreconditioned and right-preconditioned, for non-symmetric systems, gfx950.
//
// An EXTENSION: the reference's only solver is ConjugateGradient (linearsolver.rs:12-61); bicgstab.hip is the library's short
// recurrence for matrices that are not symmetric, and this is the robust one: it cannot break down before the Krylov space is
// exhausted and it does not stagnate where BiCGSTAB's omega goes to zero (a spectrum near the imaginary axis).  The family's
// conventions: the guards of linearsolver.rs:30-36, no stop test before the first body, one rounding per operation (p_mul / p_add /
// p_div; sqrt is IEEE's, correctly rounded; a - b*c is add(a, -mul(b, c)); nothing is contracted), products by the matrix's own
// kernel.  `restart` is m, 1 <= m <= 128 (kGmMaxM); 0 stands for 30.
//   set-up:  r = b - A x;  rr = r.r;  beta = sqrt(rr)
//            beta == 0: stop, no body entered, breakdown 2 (also when iter_max == 0)
//            v_0 = r / beta;  g = (beta);  j = 0;  cycles = 1
//   body (iters += 1; columns v_0 .. v_j exist):
//      w = A v_j
//      pass 1:  h1_c = v_c.w  (c = 0 .. j, all from the same w);  w = (..((w - v_0 h1_0) - v_1 h1_1) .. - v_j h1_j)   ascending c
//      pass 2:  h2_c = v_c.w;  the same update with h2                                  (classical Gram-Schmidt, twice)
//      h_c = h1_c + h2_c;  hn = sqrt(w.w)                                               (hn is h_{j+1,j})
//      the stored rotations i = 0 .. j-1 on (h_i, h_{i+1}):  t = c_i h_i + s_i h_{i+1};  h_{i+1} = (-s_i) h_i + c_i h_{i+1};  h_i = t
//      d = sqrt(h_j h_j + hn hn);  c_j = h_j / d;  s_j = hn / d;  R[0..j, j] = (h_0 .. h_{j-1}, c_j h_j + s_j hn)
//      g_{j+1} = (-s_j) g_j;  g_j = c_j g_j;  j += 1
//      v_j = w / hn  (element by element, a division), or w itself when hn == 0   -- in EVERY entered body, a cycle's last too
//      the cycle ends when   hn == 0               (breakdown 1: the Krylov space is exhausted; x is updated from it)
//                       or   |f64(g_j)| < tol      (converged)
//                       or   iters == iter_max
//                       or   j == m                (restart -- only if none of the three above holds: they stop the solve)
//      Any of them ends the cycle; breakdown 1 is reported whenever hn == 0, also when |g_j| < tol holds with it (A = 2 I).
//   cycle end:  R y = g[0..j) by back substitution: i descending, y_i = ((..(g_i - R_{i,i+1} y_{i+1}) - ..) - R_{i,j-1} y_{j-1}) / R_ii
//               x = (..((x + v_0 y_0) + v_1 y_1) .. + v_{j-1} y_{j-1})
//               z = (0, .., 0, g_j);  i = j-1 .. 0 on (z_i, z_{i+1}):  t = c_i z_i + (-s_i) z_{i+1};  z_{i+1} = s_i z_i + c_i z_{i+1};  z_i = t
//               r = (..(v_0 z_0 + v_1 z_1) .. + v_j z_j);  rr = r.r             (the residual's coordinates in v_0 .. v_j)
//               on a restart:  beta = sqrt(rr);  beta == 0: stop, breakdown 2;  else v_0 = r / beta, g = (beta), j = 0, cycles += 1
// No product at a cycle end: the residual is rebuilt from the basis (CG and BiCGSTAB trust their recurrence residual too), so a
// solve is one fixed chain of launches.  Two Gram-Schmidt passes keep max|V^T V - I| at working precision (one pass lets it grow to
// 0.09 in f32 at m = 30: not offered).  d is NOT scaled against overflow, and a singular matrix gives IEEE values (c_j = 0 / 0), not
// an error.  The comparisons with zero are exact and NaN compares false, so non-finite data run to iter_max (restarting on the way).
// Outputs: iters = bodies entered; rr = the last rebuilt r.r (the initial residual's before the first cycle end); cycles = the
// number of times a v_0 was formed; breakdown 0, 1 or 2.
//
// Storage: the basis is m + 1 columns of n, column-major, the column stride rounded up to 16 bytes (ld), so every column is a
// vector that 16-byte loads sweep.  The product reads its input at a fixed address (the graph of a batch is replayed), so the
// normalising sweep writes the new vector twice: to its column and to `vin` (n values more per body than a pointer would cost).
// Kernels: beside the product a body at column j is  dots (j + 2 vectors read) - fold - update (j + 2 read, 1 written), twice;
// the step (one workgroup: folds w.w, thread 0 does the rotations and the decisions and, at a cycle end, y and z); the
// normalisation (1 read, 2 written): (4 j + 13) n values, (2 m + 11) n averaged over a full cycle.  A cycle end adds one sweep over
// the basis that forms x and r with the partials of r.r ((j + 2) read, 2 written), its fold, and on a restart v_0 (1 read, 2 written).
// Every sweep is solver_tree.hpp's sweep, a column of the basis being one more array to load from.
// The dots (krylov_sweeps.hpp): w's pack is loaded once per tile of kGsTile = 8 columns, one accumulator per column; every column is summed by
// solver_tree.hpp's tree on pcg_grid(n) -- cg_model.Reducer.dot(., ., "pcg") -- so the tile width changes no bit.
// All state is on the device: a leading block in CgScalars' layout (solve_in_batches polls it; `converged` means STOPPED) and a
// second block (GmMore).  The kernels read the column count from it; a sweep that is not due returns at once: the Gram-Schmidt
// sweeps when the body will not be entered (stopped, or iter_max bodies entered -- `iters` moves only in the step), the others on
// the gate words the step and the cycle end's fold leave.  Bodies enqueued past the stop are no-ops.  No float atomics.
//
// Right-preconditioned (smh_gmres_precond_solve*): A M^-1 u = b, x = M^-1 u, so the residual that is minimised is the true one and
// the stop rule, rr, cycles and both codes keep their meaning.  What changes in the recurrence above:
//   set-up:     nothing (r = b - A x; M is not applied to the residual)
//   body:       u = M^-1 v_j;  w = A u        (both Gram-Schmidt passes, the step and v_{j+1} = w / hn as above)
//   cycle end:  t = (..(v_0 y_0 + v_1 y_1) .. + v_{j-1} y_{j-1})   (starts from the product, as r does);  q = M^-1 t;  x = x + q
//               (r, rr and the restart as above: rebuilt from the basis, no product)
// The driver is instantiated per PrecondShape (precond.hpp); kPcNone's chain of launches is the one described above, launch for launch.
// kPcFused (Jacobi): M^-1 v is v_i / d_i, a division, d_i the first stored (i, i) (precond.hpp's probe, as Jacobi-PCG forms z), and costs no
// launch: both forms of the normalising sweep write v to its column and v / d to the product's fixed input, the cycle end's sweep
// keeps t in registers and stores x + t / d.  One read of d each: a body at column j moves (4 j + 14) n values beside the product, a
// cycle end and a restart's v_0 one more each; (m + 6) n values of storage.
// kPcLaunched: M^-1 is applied by launches of its own (Precond, precond.hpp); for SGS on the matrix itself and ILU(0) on a factor, two
// level-scheduled triangular solves on one handle.  The body's chain opens with the application vin -> u (the product then reads u); the cycle end's sweep writes t where
// w was (w is free once v_{j+1} is formed) and r with the partials of r.r, one application t -> q follows in place, then the sweep
// x += q.  Every triangular launch takes a device gate word: the cycle end's is do_end, the body's is GmMore::enter -- "the next body
// will be entered" -- which the set-up's and the restart's k_gm_begin and every k_gm_step leave (iters == iter_max is a stop, so
// after a step "not stopped" says it all; the set-up compares with iter_max itself), so bodies enqueued past the stop run no solve.
// (m + 7) n values of storage.  A captured batch holds two applications per body: the node budget (bodies_within_budget, precond.hpp)
// makes the batches smaller or drops the capture, which changes no bit.
// rr is the RECURRENCE residual's r.r: where the solves amplify rounding it parts from |b - A x|^2.
// A pair of product handles (smh_gmres_fsai_solve*: M^-1 v = gt (g v), fsai.hip's factors) runs the same chain with Precond's products, and
// the same (m + 7) n values: no vector more.  The body's application vin -> u is two products through the handles' own AUTO kernels,
// ungated as the body's own product is: past the stop they form the same u from the same vin again.  The cycle end's q = M^-1 t is
// formed by two GATED storage-order products (precond.hpp's k_gated_seq on do_end: w -> tw -> w, SMH_SPMV_SEQ's bits), which return
// at once in a body that ends no cycle -- through AUTO every body would pay a second, dead pair.  So q has SEQ's bits and u AUTO's.
#include "internal.hpp"
#include "precond.hpp"
#include "krylov_sweeps.hpp"
#include "solver_host.hpp"
#include "solver_tree.hpp"

#include <cmath>

using namespace smh;

namespace {

constexpr int kGmMaxM = 128;
constexpr size_t kGmDefaultRestart = 30;

// the block the host polls through CG's reader (cg_read_scalars)
template <typename T>
struct GmScalars {
    T rr, spare0_, spare1_, spare2_, spare3_;
    uint32_t converged;  // STOPPED: converged, a breakdown
    uint32_t spare4_, spare5_, pad_;
    uint64_t iters;
    uint64_t iter_max;
    double tol;
};
static_assert(scalars_like_cg<GmScalars>(), "GmScalars and CgScalars have drifted apart");

// the solver's further state; the host reads the words before `hn` once, after the loop
template <typename T>
struct GmMore {
    uint32_t j;          // columns v_0 .. v_j exist
    uint32_t m;          // restart
    uint32_t cycles;
    uint32_t breakdown;  // 0 none, 1 hn == 0, 2 beta == 0
    uint32_t do_norm;    // gate: this body's normalisation is due
    uint32_t do_end;     // gate: a cycle end is due (the x / r sweep and its fold)
    uint32_t do_v0;      // gate: a restart is due (v_0 = r / beta)
    uint32_t restart;    // the cycle end that is due is a restart (not a stop)
    uint32_t enter;      // gate: the next body will be entered (the application that opens it is due)
    T hn, beta;
    T g[kGmMaxM + 1], c[kGmMaxM], s[kGmMaxM], h1[kGmMaxM + 1], h2[kGmMaxM + 1], y[kGmMaxM], z[kGmMaxM + 1];
    T R[kGmMaxM * kGmMaxM];  // R_{i,k} at [k * kGmMaxM + i], i <= k
};

template <typename T> __device__ __forceinline__ bool gm_enters(const GmScalars<T> *sc) { return !sc->converged && sc->iters < sc->iter_max; }

template <typename T>
__global__ void k_gm_init(GmScalars<T> *sc, GmMore<T> *mo, double tol, uint64_t iter_max, uint32_t m) {
    sc->rr = sc->spare0_ = sc->spare1_ = sc->spare2_ = sc->spare3_ = T(0);
    sc->converged = sc->spare4_ = sc->spare5_ = sc->pad_ = 0;
    sc->iters = 0;
    sc->iter_max = iter_max;
    sc->tol = tol;
    mo->j = mo->cycles = mo->breakdown = mo->do_norm = mo->do_end = mo->do_v0 = mo->restart = mo->enter = 0;
    mo->m = m;
    mo->hn = mo->beta = T(0);
}

// ---- the sweeps over the basis (basis: columns of stride ld, ld % V == 0) ------------------------------------------------------
// The Gram-Schmidt sweeps -- dots, folds, update -- are krylov_sweeps.hpp's (eigsh.hip runs the same ones).  Their "is due" word is
// GmMore::enter: the set-up's and the restart's k_gm_begin and every k_gm_step leave it equal to gm_enters(sc).
// partials of r.r (set-up)
template <typename T>
__global__ void __launch_bounds__(kBlock) k_gm_rr(const T *__restrict__ r, uint64_t n, T *__restrict__ part) {
    block_partial(sweep_dot(r, r, n), part);
}

// V0 false: v_j = w / hn (w itself when hn == 0), to its column and to vin.  V0 true: v_0 = r / beta, the same two places.
// kPcFused: vin takes u = v / diag, the product's input, instead
template <typename T, bool V0, PrecondShape P = kPcNone>
__global__ void __launch_bounds__(kBlock)
k_gm_norm(const GmMore<T> *__restrict__ mo, const T *__restrict__ src, T *__restrict__ basis, uint64_t ld, T *__restrict__ vin, uint64_t n,
          const T *__restrict__ diag = nullptr) {
    if (!(V0 ? mo->do_v0 : mo->do_norm)) return;
    const T d = V0 ? mo->beta : mo->hn;
    const bool copy = !V0 && d == T(0);
    T *__restrict__ colp = basis + (V0 ? (uint64_t)0 : (uint64_t)mo->j * ld);  // (the step has advanced j: at most m)
    sweep<T>(n, [&](auto at) {
        auto v = at.load(src);
        if (!copy) {
#pragma unroll
            for (int e = 0; e < at.width; ++e) v[e] = p_div(v[e], d);
        }
        at.store(colp, v);
        if constexpr (P == kPcFused) {
            const auto dv = at.load(diag);
#pragma unroll
            for (int e = 0; e < at.width; ++e) v[e] = p_div(v[e], dv[e]);
        }
        at.store(vin, v);
    });
}

// the cycle end: x += sum v_c y_c (c < j), r = sum v_c z_c (c <= j), the partials of r.r.  Preconditioned, the sum t starts from
// its first product and stays out of x: kPcFused keeps it in registers and stores x + t / diag; kPcLaunched writes it to t_out (x is
// not touched: x += M^-1 t follows)
template <typename T, PrecondShape P = kPcNone>
__global__ void __launch_bounds__(kBlock)
k_gm_xr(const GmMore<T> *__restrict__ mo, const T *__restrict__ basis, uint64_t ld, T *__restrict__ x, T *__restrict__ r, uint64_t n, T *__restrict__ part_rr,
        const T *__restrict__ diag = nullptr, T *__restrict__ t_out = nullptr) {
    if (!mo->do_end) return;
    const unsigned j = mo->j;  // >= 1
    const T *__restrict__ y = mo->y, *__restrict__ z = mo->z;
    T acc = T(0);
    sweep<T>(n, [&](auto at) {
        typename decltype(at)::pack xv, rv;  // xv: x and its sum, or (preconditioned) t
        if constexpr (P == kPcNone) xv = at.load(x);
        {
            const auto vv = at.load(basis);
            const T y0 = y[0], z0 = z[0];
#pragma unroll
            for (int e = 0; e < at.width; ++e) {
                if constexpr (P == kPcNone) xv[e] = p_add(xv[e], p_mul(vv[e], y0));
                else xv[e] = p_mul(vv[e], y0);
                rv[e] = p_mul(vv[e], z0);
            }
        }
#pragma unroll 4
        for (unsigned c = 1; c < j; ++c) {
            const auto vv = at.load(basis + (uint64_t)c * ld);
            const T yc = y[c], zc = z[c];
#pragma unroll
            for (int e = 0; e < at.width; ++e) {
                xv[e] = p_add(xv[e], p_mul(vv[e], yc));
                rv[e] = p_add(rv[e], p_mul(vv[e], zc));
            }
        }
        {
            const auto vv = at.load(basis + (uint64_t)j * ld);
            const T zj = z[j];
#pragma unroll
            for (int e = 0; e < at.width; ++e) {
                rv[e] = p_add(rv[e], p_mul(vv[e], zj));
                acc = p_add(acc, p_mul(rv[e], rv[e]));
            }
        }
        if constexpr (P == kPcFused) {
            const auto x0 = at.load(x), dv = at.load(diag);
#pragma unroll
            for (int e = 0; e < at.width; ++e) xv[e] = p_add(x0[e], p_div(xv[e], dv[e]));
        }
        at.store(P == kPcLaunched ? t_out : x, xv);
        at.store(r, rv);
    });
    block_partial(acc, part_rr);
}

// kPcLaunched's last sweep of a cycle end: x = x + q, q = M^-1 t
template <typename T>
__global__ void __launch_bounds__(kBlock) k_gm_xadd(const GmMore<T> *__restrict__ mo, T *__restrict__ x, const T *__restrict__ q, uint64_t n) {
    if (!mo->do_end) return;
    sweep<T>(n, [&](auto at) {
        auto xv = at.load(x);
        const auto qv = at.load(q);
#pragma unroll
        for (int e = 0; e < at.width; ++e) xv[e] = p_add(xv[e], qv[e]);
        at.store(x, xv);
    });
}

// ---- the one-workgroup kernels ----------------------------------------------------------------------------------------------------
// rr = r.r.  SETUP: of the initial residual, and the first cycle begins.  Else: of the rebuilt one, and on a restart the next begins.
// beta = sqrt(rr);  beta == 0: stop, breakdown 2;  else g = (beta), j = 0, cycles += 1, v_0 is due
template <typename T, bool SETUP>
__global__ void __launch_bounds__(kBlock) k_gm_begin(GmScalars<T> *sc, GmMore<T> *mo, const T *__restrict__ part, unsigned n_parts) {
    if (!SETUP && !mo->do_end) return;
    const T rr = fold1(part, n_parts);
    if (threadIdx.x == 0) {
        sc->rr = rr;
        mo->do_v0 = 0;
        if (SETUP || mo->restart) {
            const T beta = p_sqrt(rr);
            if (beta == T(0)) {
                mo->breakdown = 2;
                sc->converged = 1;
            } else {
                mo->beta = beta;
                mo->g[0] = beta;
                mo->j = 0;
                mo->cycles += 1;
                mo->do_v0 = 1;
            }
            mo->enter = gm_enters(sc) ? 1u : 0u;  // (a restart follows a step that stopped nothing: beta == 0 alone closes the gate)
        }
    }
}

// the body's sequential part: decides whether the body counts, folds w.w, the rotations, the decisions, y and z at a cycle end
template <typename T>
__global__ void __launch_bounds__(kBlock) k_gm_step(GmScalars<T> *sc, GmMore<T> *mo, const T *__restrict__ part_ww, unsigned n_parts) {
    if (!gm_enters(sc)) {  // (every thread reads before thread 0 writes: the fold below has a barrier)
        if (threadIdx.x == 0) mo->do_norm = mo->do_end = mo->do_v0 = mo->enter = 0;
        return;
    }
    const T ww = fold1(part_ww, n_parts);
    if (threadIdx.x != 0) return;
    const uint64_t iters = sc->iters + 1;
    sc->iters = iters;
    unsigned j = mo->j;
    T *h = mo->h1;
    for (unsigned c = 0; c <= j; ++c) h[c] = p_add(mo->h1[c], mo->h2[c]);
    const T hn = p_sqrt(ww);
    for (unsigned i = 0; i < j; ++i) {
        const T ci = mo->c[i], si = mo->s[i], a = h[i], b = h[i + 1];
        h[i] = p_add(p_mul(ci, a), p_mul(si, b));
        h[i + 1] = p_add(p_mul(-si, a), p_mul(ci, b));
    }
    const T hj = h[j];
    const T d = p_sqrt(p_add(p_mul(hj, hj), p_mul(hn, hn)));
    const T cj = p_div(hj, d), sj = p_div(hn, d);
    mo->c[j] = cj;
    mo->s[j] = sj;
    T *Rj = mo->R + (size_t)j * kGmMaxM;
    for (unsigned i = 0; i < j; ++i) Rj[i] = h[i];
    Rj[j] = p_add(p_mul(cj, hj), p_mul(sj, hn));
    const T gj = mo->g[j];
    const T gn = p_mul(-sj, gj);
    mo->g[j + 1] = gn;
    mo->g[j] = p_mul(cj, gj);
    j += 1;
    mo->j = j;
    mo->hn = hn;
    mo->do_norm = 1;
    mo->do_v0 = 0;
    const bool exhausted = hn == T(0), conv = fabs((double)gn) < sc->tol, last = iters == sc->iter_max, full = j == mo->m;
    const bool stop = exhausted || conv || last;
    mo->enter = stop ? 0u : 1u;  // (iters == iter_max is a stop)
    if (!(stop || full)) {
        mo->do_end = 0;
        return;
    }
    mo->do_end = 1;
    mo->restart = stop ? 0 : 1;
    if (exhausted) mo->breakdown = 1;
    if (stop) sc->converged = 1;
    // R y = g[0 .. j)
    for (int i = (int)j - 1; i >= 0; --i) {
        T a = mo->g[i];
        for (unsigned k = i + 1; k < j; ++k) a = p_add(a, -p_mul(mo->R[(size_t)k * kGmMaxM + i], mo->y[k]));
        mo->y[i] = p_div(a, mo->R[(size_t)i * kGmMaxM + i]);
    }
    // z = Omega_0^T .. Omega_{j-1}^T (g_j e_j)
    for (unsigned i = 0; i < j; ++i) mo->z[i] = T(0);
    mo->z[j] = gn;
    for (int i = (int)j - 1; i >= 0; --i) {
        const T ci = mo->c[i], si = mo->s[i], a = mo->z[i], b = mo->z[i + 1];
        mo->z[i] = p_add(p_mul(ci, a), p_mul(-si, b));
        mo->z[i + 1] = p_add(p_mul(si, a), p_mul(ci, b));
    }
}

// P: precond_shape(pc).  kPcNone's chain of launches is the unpreconditioned solver's, launch for launch.
template <typename T, PrecondShape P>
int gmres_t(smh_crs *m, const Precond &pc, const SolveCall &c) {
    const int dt = sizeof(T) == 8 ? SMH_F64 : SMH_F32;
    constexpr size_t V = 16 / sizeof(T);
    const size_t n = c.n, restart = c.restart;
    SolveRun run;  // (its `converged` means STOPPED here)
    int breakdown = 0;
    size_t cycles = 0;
    const unsigned grid = pcg_grid(n);
    const uint64_t ld = (n + V - 1) / V * V;
    const int rc = run.run([&]() -> int {
        SMH_TRY(precond_prepare(pc));
        SMH_TRY(run.own_stream());
        const hipStream_t s = run.s;
        Scratch &ws = run.ws;
        T *x = nullptr, *r = nullptr, *w = nullptr, *vin = nullptr, *basis = nullptr, *part = nullptr, *part_ww = nullptr;
        T *diag = nullptr, *u = nullptr, *tw = nullptr;  // fused: the diagonal.  Launched: u = M^-1 v_j and the application's scratch
        GmScalars<T> *sc = nullptr;
        GmMore<T> *mo = nullptr;
        SMH_TRY(ws.alloc(&x, n)); SMH_TRY(ws.alloc(&r, n)); SMH_TRY(ws.alloc(&w, n)); SMH_TRY(ws.alloc(&vin, n));
        SMH_TRY(ws.alloc(&basis, (restart + 1) * (size_t)ld));
        SMH_TRY(ws.alloc(&part, (restart + 1) * (size_t)kPcgBlocks));
        SMH_TRY(ws.alloc(&part_ww, (size_t)kPcgBlocks));
        SMH_TRY(ws.alloc(&sc, 1));
        SMH_TRY(ws.alloc(&mo, 1));
        constexpr size_t more_head = offsetof(GmMore<T>, hn);
        SMH_TRY(run.h_sc.alloc(sizeof(GmScalars<T>) + more_head, hipHostMallocDefault));
        if constexpr (P == kPcFused) SMH_TRY(ws.alloc(&diag, n));
        if constexpr (P == kPcLaunched) { SMH_TRY(ws.alloc(&u, n)); SMH_TRY(ws.alloc(&tw, n)); }
        SMH_TRY(precond_setup(pc, n, P == kPcFused ? diag : u, ws, s));  // (u: the solves' probe keeps no values)
        // r = b - A x (w: scratch); rr = r.r; beta; v_0
        hipLaunchKernelGGL((k_gm_init<T>), dim3(1), dim3(1), 0, s, sc, mo, c.tol, (uint64_t)c.iter_max, (uint32_t)restart);
        SMH_TRY(stage_residual(m, c.variant, (const T *)c.b, (const T *)c.x, n, r, x, w, s));
        hipLaunchKernelGGL((k_gm_rr<T>), dim3(grid), dim3(kBlock), 0, s, r, (uint64_t)n, part_ww);
        hipLaunchKernelGGL((k_gm_begin<T, true>), dim3(1), dim3(kBlock), 0, s, sc, mo, part_ww, grid);
        hipLaunchKernelGGL((k_gm_norm<T, true, P>), dim3(grid), dim3(kBlock), 0, s, mo, r, basis, ld, vin, (uint64_t)n, diag);
        SMH_HIP(hipGetLastError());
        const dim3 cols((unsigned)restart + 1);
        auto body = [&]() -> int {
            if constexpr (P == kPcLaunched) {
                SMH_TRY(precond_apply_enqueue(pc, vin, tw, u, &mo->enter, s));
                SMH_TRY(spmv_enqueue(m, u, n, w, c.variant, s));
            } else {
                SMH_TRY(spmv_enqueue(m, vin, n, w, c.variant, s));
            }
            hipLaunchKernelGGL((k_gs_dots<T>), dim3(grid), dim3(kBlock), 0, s, &mo->enter, &mo->j, basis, ld, w, (uint64_t)n, part);
            hipLaunchKernelGGL((k_gs_fold<T>), cols, dim3(kBlock), 0, s, &mo->enter, &mo->j, mo->h1, part, grid);
            hipLaunchKernelGGL((k_gs_update<T, false>), dim3(grid), dim3(kBlock), 0, s, &mo->enter, &mo->j, mo->h1, basis, ld, w, (uint64_t)n, part_ww);
            hipLaunchKernelGGL((k_gs_dots<T>), dim3(grid), dim3(kBlock), 0, s, &mo->enter, &mo->j, basis, ld, w, (uint64_t)n, part);
            hipLaunchKernelGGL((k_gs_fold<T>), cols, dim3(kBlock), 0, s, &mo->enter, &mo->j, mo->h2, part, grid);
            hipLaunchKernelGGL((k_gs_update<T, true>), dim3(grid), dim3(kBlock), 0, s, &mo->enter, &mo->j, mo->h2, basis, ld, w, (uint64_t)n, part_ww);
            hipLaunchKernelGGL((k_gm_step<T>), dim3(1), dim3(kBlock), 0, s, sc, mo, part_ww, grid);
            hipLaunchKernelGGL((k_gm_norm<T, false, P>), dim3(grid), dim3(kBlock), 0, s, mo, w, basis, ld, vin, (uint64_t)n, diag);
            hipLaunchKernelGGL((k_gm_xr<T, P>), dim3(grid), dim3(kBlock), 0, s, mo, basis, ld, x, r, (uint64_t)n, part_ww, diag, w);  // (w is free)
            hipLaunchKernelGGL((k_gm_begin<T, false>), dim3(1), dim3(kBlock), 0, s, sc, mo, part_ww, grid);
            if constexpr (P == kPcLaunched) {  // q = M^-1 t in place, x += q: due at a cycle end alone
                SMH_TRY(precond_apply_gated_enqueue(pc, w, tw, w, &mo->do_end, s));
                hipLaunchKernelGGL((k_gm_xadd<T>), dim3(grid), dim3(kBlock), 0, s, mo, x, w, (uint64_t)n);
            }
            hipLaunchKernelGGL((k_gm_norm<T, true, P>), dim3(grid), dim3(kBlock), 0, s, mo, r, basis, ld, vin, (uint64_t)n, diag);
            SMH_HIP(hipGetLastError());
            return SMH_OK;
        };
        if constexpr (P == kPcLaunched) {
            // the node budget of a captured batch: two applications, the product (a few nodes at most) and the chain of 12
            bool capture = true;
            const size_t bodies = bodies_within_budget(2 * precond_apply_nodes(pc) + 1 + 3 + 12, c.check_every, &capture);
            SMH_TRY(run.loop(dt, c.iter_max, bodies, body, sc, capture));
        } else {
            SMH_TRY(run.loop(dt, c.iter_max, c.check_every, body, sc));
        }
        GmMore<T> *h_mo = (GmMore<T> *)((char *)run.h_sc.get() + sizeof(GmScalars<T>));  // (its head alone)
        SMH_HIP(hipMemcpyAsync(h_mo, mo, more_head, hipMemcpyDeviceToHost, s));
        if (n) SMH_HIP(hipMemcpyAsync(c.x, x, n * sizeof(T), hipMemcpyDefault, s));
        SMH_HIP(hipStreamSynchronize(s));
        breakdown = (int)h_mo->breakdown;
        cycles = (size_t)h_mo->cycles;
        return SMH_OK;
    }, c.iters_out, c.rr_out);
    if (rc == SMH_OK && c.breakdown_out) *c.breakdown_out = breakdown;
    if (rc == SMH_OK && c.cycles_out) *c.cycles_out = cycles;
    return rc;
}

// the handles' check, then the driver of the matrix's dtype and the preconditioner's shape
int gmres(smh_crs *m, const Precond &pc, const SolveCall &c) {
    SMH_TRY(precond_check_handles(pc));
    return with_dtype_and_shape(m->dtype, precond_shape(pc), [&](auto t, auto shape) { return gmres_t<decltype(t), decltype(shape)::value>(m, pc, c); });
}

constexpr size_t kGmCheckEvery = 8;  // bodies per poll that check_every = 0, and the host form, stand for

}  // namespace

// the statuses are decided here (solver_host.hpp), before any launch: BiCGSTAB's, then the range of `restart`
extern "C" int smh_gmres_solve_vec(smh_crs *m, const smh_vec *b, smh_vec *x, double tol, size_t iter_max, size_t restart, int variant,
                                   size_t check_every, size_t *iters_out, double *rr_out, size_t *cycles_out, int *breakdown_out) {
    SMH_TRY(check_solve_vec(m, b, x, kVecDtype, /*refuse_aliased*/ true, &check_every, kGmCheckEvery));
    SMH_TRY(check_solve_restart(&restart, kGmDefaultRestart, kGmMaxM));
    return gmres(m, no_precond(), {b->d, x->d, m->n_rows, tol, iter_max, variant, check_every, iters_out, rr_out, breakdown_out, restart, cycles_out});
}

extern "C" int smh_gmres_solve(smh_crs *m, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len, double tol, size_t iter_max,
                               size_t restart, int variant, size_t *iters_out, double *rr_out, size_t *cycles_out, int *breakdown_out) {
    SMH_TRY(check_solve_host(m, b_host, b_len, x_host_inout, x_len, /*null_vectors*/ true, /*refuse_aliased*/ true));
    SMH_TRY(check_solve_restart(&restart, kGmDefaultRestart, kGmMaxM));
    return gmres(m, no_precond(), {b_host, x_host_inout, m->n_rows, tol, iter_max, variant, kGmCheckEvery, iters_out, rr_out, breakdown_out, restart, cycles_out});
}

// Right-preconditioned: `precond` and `f` first (check_precond, precond.hpp), then the checks above (with ILU's factor against the matrix, as smh_pcg_ilu_solve);
// what needs the device -- a stored column >= n, a zero or absent diagonal entry -- is decided in the driver before its first launch
extern "C" int smh_gmres_precond_solve_vec(smh_crs *a, int precond, smh_crs *f, const smh_vec *b, smh_vec *x, double tol, size_t iter_max,
                                           size_t restart, int variant, size_t check_every, size_t *iters_out, double *rr_out, size_t *cycles_out,
                                           int *breakdown_out) {
    SMH_TRY(check_precond(precond, f));
    if (precond == SMH_PRECOND_NONE) return smh_gmres_solve_vec(a, b, x, tol, iter_max, restart, variant, check_every, iters_out, rr_out, cycles_out, breakdown_out);
    SMH_TRY(check_solve_vec(a, b, x, kVecDtype, /*refuse_aliased*/ true, &check_every, kGmCheckEvery, f));
    SMH_TRY(check_solve_restart(&restart, kGmDefaultRestart, kGmMaxM));
    return gmres(a, precond_of(precond, a, f), {b->d, x->d, a->n_rows, tol, iter_max, variant, check_every, iters_out, rr_out, breakdown_out, restart, cycles_out});
}

extern "C" int smh_gmres_precond_solve(smh_crs *a, int precond, smh_crs *f, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len,
                                       double tol, size_t iter_max, size_t restart, int variant, size_t *iters_out, double *rr_out,
                                       size_t *cycles_out, int *breakdown_out) {
    SMH_TRY(check_precond(precond, f));
    if (precond == SMH_PRECOND_NONE) return smh_gmres_solve(a, b_host, b_len, x_host_inout, x_len, tol, iter_max, restart, variant, iters_out, rr_out, cycles_out, breakdown_out);
    SMH_TRY(check_solve_host(a, b_host, b_len, x_host_inout, x_len, /*null_vectors*/ true, /*refuse_aliased*/ true, f));
    SMH_TRY(check_solve_restart(&restart, kGmDefaultRestart, kGmMaxM));
    return gmres(a, precond_of(precond, a, f),
                 {b_host, x_host_inout, a->n_rows, tol, iter_max, variant, kGmCheckEvery, iters_out, rr_out, breakdown_out, restart, cycles_out});
}

// Right-preconditioned by a pair of product handles, M^-1 v = gt (g v): (G_L, G_U) of smh_crs_fsai_ns, or (G, G^T) of smh_crs_fsai for
// a symmetric a.  The pair's checks are smh_pcg_fsai_solve's, then the restart's; nothing is probed (no operation divides by a factor's
// value); a stored column >= n is decided in the driver before its first launch
extern "C" int smh_gmres_fsai_solve_vec(smh_crs *a, smh_crs *g, smh_crs *gt, const smh_vec *b, smh_vec *x, double tol, size_t iter_max, size_t restart,
                                        int variant, size_t check_every, size_t *iters_out, double *rr_out, size_t *cycles_out, int *breakdown_out) {
    SMH_TRY(check_pair_vec(a, g, gt, kFsaiName, b, x, &check_every, kGmCheckEvery));
    SMH_TRY(check_solve_restart(&restart, kGmDefaultRestart, kGmMaxM));
    return gmres(a, fsai_precond(g, gt), {b->d, x->d, a->n_rows, tol, iter_max, variant, check_every, iters_out, rr_out, breakdown_out, restart, cycles_out});
}

extern "C" int smh_gmres_fsai_solve(smh_crs *a, smh_crs *g, smh_crs *gt, const void *b_host, size_t b_len, void *x_host_inout, size_t x_len, double tol,
                                    size_t iter_max, size_t restart, int variant, size_t *iters_out, double *rr_out, size_t *cycles_out,
                                    int *breakdown_out) {
    SMH_TRY(check_pair_host(a, g, gt, kFsaiName, b_host, b_len, x_host_inout, x_len, /*refuse_aliased*/ true));
    SMH_TRY(check_solve_restart(&restart, kGmDefaultRestart, kGmMaxM));
    return gmres(a, fsai_precond(g, gt),
                 {b_host, x_host_inout, a->n_rows, tol, iter_max, variant, kGmCheckEvery, iters_out, rr_out, breakdown_out, restart, cycles_out});
}
