// eigsh.hip -- thick-restart Lanczos (Wu & Simon) with full reorthogonalisation: the k algebraically largest or smallest eigenpairs
// of a symmetric matrix, gfx950.
//
// An EXTENSION: the reference has no eigensolver (its only solver is ConjugateGradient, linearsolver.rs:12-61).  SYMMETRY IS THE
// CALLER'S PROMISE, as it is for CG: nothing checks it, and on a matrix that is not symmetric the numbers returned mean nothing.
// A MULTIPLE EIGENVALUE IS FOUND ONCE, as in any single-vector Lanczos: the Krylov space of one start vector holds one direction of
// its eigenspace.  The family's conventions: one rounding per operation (p_mul / p_add / p_div; sqrt is IEEE's, correctly rounded;
// a - b*c is add(a, -mul(b, c)); nothing is contracted), comparisons with zero are exact, products by the matrix's own kernel.
//   parameters: k >= 1;  m ("ncv"), clipped to n, k + 2 <= m <= 128 (0: the default, min(n, max(2k + 1, 20)));  whenever k + 2 > n: m = n;
//               which in {LARGEST, SMALLEST};  tol;  restart_max;  a start vector v (n values)
//   set-up:     nv = sqrt(v.v);  nv == 0 or non-finite: breakdown 2, nothing returned;  v_0 = v / nv;  l = 0
//   body at column j (l <= j < m), products += 1:
//               w = A v_j
//               pass 1: h1_c = v_c.w (c = 0..j, all from the same w);  w = (..(w - v_0 h1_0) .. - v_j h1_j)  ascending
//               pass 2: h2_c = v_c.w;  the same update                 (classical Gram-Schmidt twice: GMRES's sweeps)
//               alpha_j = h1_j + h2_j;  beta_j = sqrt(w.w);  v_{j+1} = w / beta_j   (element by element)
//               beta_j == 0: the Krylov space is exhausted (breakdown 1): the cycle ends with j + 1 columns
//   projected matrix (arrowhead + tridiagonal, in T):
//               diag = (theta_0..theta_{l-1}, alpha_l..alpha_{m-1});  (i, l) = (l, i) = s_i for i < l;
//               (j, j+1) = (j+1, j) = beta_j for l <= j < m - 1.  The other h_c are rounding-level and are NOT stored.
//   cycle end (one host round trip): alpha, beta, s, theta widened to f64; cyclic Jacobi in f64 (eigsh_host.hpp) -> theta (ascending,
//               ties by index), Y (m x m).  Order the Ritz pairs wanted-first.  est_i = |f64(beta_{m-1}) * Y[m-1, i]|;
//               pair i is converged when est_i <= tol * max_c |theta_c|  (over all m Ritz values);
//               n_conv = the length of the converged PREFIX of the wanted order.
//               stop when n_conv == k, or restarts == restart_max, or m == n, or breakdown 1, or any alpha / beta is non-finite
//               (breakdown 3).  Else restart:  l = k + (m - k) / 2  (integer division);  Yt = T(Y[:, first l wanted])
//               v_i (i < l) = (..(v_0 Yt[0,i] + v_1 Yt[1,i]) .. + v_{m-1} Yt[m-1,i])   -- starts from the product, ascending
//               v_l = v_m;  theta_i = T(theta_i);  s_i = beta_{m-1} * Yt[m-1, i];  restarts += 1;  continue at j = l
//   at the stop: the first k wanted Ritz vectors by the same rotation, written to the output; eigenvalues and estimates in f64.
// The eigenvectors are not renormalised: |x_i| = 1 within the bound the depth of the sums gives.
// The corners the recurrence leaves open, decided here and in tests/eigsh_model.py:
//   - wanted-first: SMALLEST takes theta ascending (index 0, 1, ..), LARGEST the same list reversed (so ties go by index descending).
//   - "non-finite" covers every entry of the projected matrix (theta, s, alpha, beta of the cycle): breakdown 3 is decided on the host
//     before the Jacobi step, which never sees a non-finite value.  NaN compares false, so such a cycle runs its m - l bodies.
//   - breakdowns 2 and 3 return NOTHING: evals, estimates and vectors are not written, n_conv = 0; restarts and products are.
//   - after breakdown 1 the cycle has mc = j + 1 columns and beta_{mc-1} = 0: every estimate is 0, every pair converged, and the
//     min(k, mc) pairs that exist are returned; eigenvalues and estimates past them are NaN, vectors past them are the rotation by
//     zero coefficients (signed zeros); n_conv = min(k, mc).  v_{j+1} is not formed.
//   - n_conv never exceeds k; the stop conditions are tested after the estimates, so a cycle that stops for restart_max, m == n or
//     breakdown 1 reports its own n_conv.
//   - nothing is copied or rotated "in place": the basis lives in two blocks of m + 1 columns, a restart rotates from one into the
//     other (and carries v_m to column l by the same launch), and the blocks change roles.
//
// Storage: two blocks of m + 1 columns of n, column-major, the column stride rounded up to 16 bytes; w; the product's fixed input
// vin (the normalising sweep writes the new vector to its column and to vin, as gmres.hip's does); (2 m + 4) n values.
// Kernels: a body is the product, then krylov_sweeps.hpp's dots - fold - update twice (GMRES's, launch for launch), the step (one
// workgroup: folds w.w, thread 0 forms alpha_j and beta_j and advances j) and the normalisation.  The column index lives on the
// device (EgState::j) and a cycle's m - l bodies are enqueued back to back; after a breakdown the `live` word is 0 and the bodies
// that follow are no-ops.  One host round trip per cycle: the state's head and alpha / beta (16 m + 40 bytes at most) through
// pinned memory, the host step, Yt uploaded through pinned memory, the rotation.  Nothing is allocated per cycle, no graph is
// captured, no float atomics, no kernel waits for another workgroup.
// The rotation k_eg_rotate (the hot path of a restart): out_i[r] = sum_c v_c[r] Yt[c][i].  A workgroup column (blockIdx.y) owns a tile
// of kEgRotTile = 8 output columns: a thread keeps 8 packs of accumulators and every pack of V it loads (16 bytes, coalesced, as
// the sweeps read them) feeds all 8.  Yt[c][i0 .. i0+7] is uniform across the grid: the compiler reads it through scalar loads
// (s_load_dwordx8 / x16 of a row padded to the tile).  Every out_i[r] is one chain over c ascending, so no bit depends on the tile.
#include "eigsh_host.hpp"
#include "internal.hpp"
#include "krylov_sweeps.hpp"
#include "solver_host.hpp"
#include "solver_tree.hpp"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <limits>

using namespace smh;

namespace {

constexpr int kEgRotTile = 8;  // output columns per workgroup column of the rotation (no bit depends on it)

// what smh_eigsh_last_timing reports of this thread's last solve (a measuring aid: tools/eigsh_bench.py)
struct EgTiming {
    double host_ms = 0.0, rotation_ms = 0.0;
    size_t cycles = 0, rotations = 0;
};
thread_local EgTiming t_timing;
double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the solver's device state; the host reads it up to ab[2 m) once per cycle
template <typename T>
struct EgState {
    uint32_t j;          // columns v_0 .. v_j exist; the next body is column j's
    uint32_t live;       // 0: stopped (breakdown 1 or 2): every launch that follows returns at once
    uint32_t breakdown;  // 0 none, 1 beta_j == 0, 2 the start vector's norm is zero or not finite
    uint32_t do_norm;    // gate: a normalisation is due (v_j = src / nrm)
    uint64_t products;
    T nrm, spare_;
    T ab[2 * kEgMaxM];   // alpha_j, beta_j at [2 j], [2 j + 1]
    T h1[kEgMaxM + 1], h2[kEgMaxM + 1];
};

template <typename T>
__global__ void k_eg_init(EgState<T> *st) {
    st->j = st->breakdown = st->do_norm = 0;
    st->live = 1;
    st->products = 0;
    st->nrm = st->spare_ = T(0);
}

// partials of v.v (set-up)
template <typename T>
__global__ void __launch_bounds__(kBlock) k_eg_vv(const T *__restrict__ v, uint64_t n, T *__restrict__ part) {
    block_partial(sweep_dot(v, v, n), part);
}

// nv = sqrt(v.v);  zero or not finite: breakdown 2
template <typename T>
__global__ void __launch_bounds__(kBlock) k_eg_begin(EgState<T> *st, const T *__restrict__ part, unsigned n_parts) {
    const T vv = fold1(part, n_parts);
    if (threadIdx.x != 0) return;
    const T nv = p_sqrt(vv);
    if (nv == T(0) || !(fabs((double)nv) <= (double)std::numeric_limits<T>::max())) {
        st->breakdown = 2;
        st->live = 0;
    } else {
        st->nrm = nv;
        st->do_norm = 1;
    }
}

// the body's sequential part: folds w.w; alpha_j = h1_j + h2_j, beta_j = sqrt(w.w); j += 1; beta_j == 0: breakdown 1
template <typename T>
__global__ void __launch_bounds__(kBlock) k_eg_step(EgState<T> *st, const T *__restrict__ part_ww, unsigned n_parts) {
    if (!st->live) {  // (every thread reads before thread 0 writes: the fold below has a barrier)
        if (threadIdx.x == 0) st->do_norm = 0;
        return;
    }
    const T ww = fold1(part_ww, n_parts);
    if (threadIdx.x != 0) return;
    const unsigned j = st->j;
    const T beta = p_sqrt(ww);
    st->ab[2 * j] = p_add(st->h1[j], st->h2[j]);
    st->ab[2 * j + 1] = beta;
    st->products += 1;
    st->j = j + 1;
    st->nrm = beta;
    if (beta == T(0)) {
        st->breakdown = 1;
        st->live = 0;
        st->do_norm = 0;
    } else {
        st->do_norm = 1;
    }
}

// v_j = src / nrm (j as the step left it; 0 at the set-up), to its column and to vin: k_gm_norm's shape
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_eg_norm(const EgState<T> *__restrict__ st, const T *__restrict__ src, T *__restrict__ basis, uint64_t ld, T *__restrict__ vin, uint64_t n) {
    if (!st->do_norm) return;
    const T d = st->nrm;
    T *__restrict__ colp = basis + (uint64_t)st->j * ld;  // (at most column m)
    sweep<T>(n, [&](auto at) {
        auto v = at.load(src);
#pragma unroll
        for (int e = 0; e < at.width; ++e) v[e] = p_div(v[e], d);
        at.store(colp, v);
        at.store(vin, v);
    });
}

// a restart continues at column l
template <typename T>
__global__ void k_eg_restart(EgState<T> *st, uint32_t l) {
    st->j = l;
    st->do_norm = 0;
}

// out_i = (..(v_0 Yt[0][i] + v_1 Yt[1][i]) .. + v_{mc-1} Yt[mc-1][i]) for the tile i = blockIdx.y * 8 .. + 7 of the output columns
// i < cols.  yt: mc rows of ldy values (ldy % 8 == 0, zero beyond the columns that exist).
// MVEC false: out_i is column i of dst (stride ldd); the workgroup column past the last tile (carry: gridDim.y is one more) copies
// column mc of src to column cols of dst.  MVEC true: dst is an smh_mvec's interleaved storage, dst[r * ldd + i]; the padding
// columns cols <= i < ldd take +0.
template <typename T, bool MVEC>
__global__ void __launch_bounds__(kBlock)
k_eg_rotate(const T *__restrict__ src, uint64_t ld, unsigned mc, const T *__restrict__ yt, unsigned ldy, unsigned cols, T *__restrict__ dst,
            uint64_t ldd, uint64_t n, unsigned tiles) {
    if (blockIdx.y >= tiles) {  // the carry (MVEC false alone)
        const T *__restrict__ from = src + (uint64_t)mc * ld;
        T *__restrict__ to = dst + (uint64_t)cols * ldd;
        sweep<T>(n, [&](auto at) { at.store(to, at.load(from)); });
        return;
    }
    const unsigned i0 = blockIdx.y * kEgRotTile;
    const T *__restrict__ y0 = yt + i0;
    sweep<T>(n, [&](auto at) {
        typename decltype(at)::pack acc[kEgRotTile];
        {
            const auto vv = at.load(src);
#pragma unroll
            for (int t = 0; t < kEgRotTile; ++t) {
                const T y = y0[t];
#pragma unroll
                for (int e = 0; e < at.width; ++e) acc[t][e] = p_mul(vv[e], y);
            }
        }
#pragma unroll 2
        for (unsigned c = 1; c < mc; ++c) {
            const auto vv = at.load(src + (uint64_t)c * ld);
            const T *__restrict__ yc = y0 + (size_t)c * ldy;
#pragma unroll
            for (int t = 0; t < kEgRotTile; ++t) {
                const T y = yc[t];
#pragma unroll
                for (int e = 0; e < at.width; ++e) acc[t][e] = p_add(acc[t][e], p_mul(vv[e], y));
            }
        }
        if constexpr (MVEC) {
#pragma unroll
            for (int e = 0; e < at.width; ++e) {
                T *__restrict__ row = dst + (at.i + e) * ldd;
#pragma unroll
                for (int t = 0; t < kEgRotTile; ++t)
                    if (i0 + t < ldd) row[i0 + t] = i0 + t < cols ? acc[t][e] : T(0);
            }
        } else {
#pragma unroll
            for (int t = 0; t < kEgRotTile; ++t)
                if (i0 + t < cols) at.store(dst + (uint64_t)(i0 + t) * ldd, acc[t]);
        }
    });
}

// what an entry point hands the driver (the checks have passed; m is the clipped ncv)
struct EigCall {
    const void *start;  // n values of the matrix's dtype, host or device memory
    size_t n, k, m;
    int which;
    double tol;
    size_t restart_max;
    int variant;
    double *evals_out;
    void *evecs_host;   // k x n, host or device memory, or NULL
    smh_mvec *evecs;    // or NULL
    double *est_out;
    size_t *n_conv_out, *restarts_out, *products_out;
    int *breakdown_out;
};

template <typename T>
int eigsh_t(smh_crs *a, const EigCall &c) {
    constexpr size_t V = 16 / sizeof(T);
    const size_t n = c.n, m = c.m, k = c.k;
    const unsigned grid = pcg_grid(n);
    const uint64_t ld = (n + V - 1) / V * V;
    constexpr size_t kLdyMax = (kEgMaxM + kEgRotTile - 1) / kEgRotTile * kEgRotTile;
    PinnedBuf h_yt;  // (declared before the run: it outlives the stream's last copy from it, also when the solve fails half way)
    SolveRun run;
    EgHost<T> host;
    size_t restarts = 0, products = 0, kk = 0;
    int breakdown = 0;
    t_timing = EgTiming();
    const bool time_rotation = std::getenv("SMH_EIGSH_TIMING") != nullptr;  // waits for every rotation: a measuring aid, no bit moves
    const int rc = run.run([&]() -> int {
        try {
            host.init((int)k, (int)m, c.which, c.tol);
        } catch (...) {
            return fail(SMH_ERR_OOM, "host allocation failed");
        }
        SMH_TRY(run.own_stream());
        const hipStream_t s = run.s;
        Scratch &ws = run.ws;
        T *w = nullptr, *vin = nullptr, *block[2] = {nullptr, nullptr}, *part = nullptr, *part_ww = nullptr, *yt = nullptr;
        EgState<T> *st = nullptr;
        SMH_TRY(ws.alloc(&w, n)); SMH_TRY(ws.alloc(&vin, n));
        SMH_TRY(ws.alloc(&block[0], (m + 1) * (size_t)ld)); SMH_TRY(ws.alloc(&block[1], (m + 1) * (size_t)ld));
        SMH_TRY(ws.alloc(&part, (m + 1) * (size_t)kPcgBlocks));
        SMH_TRY(ws.alloc(&part_ww, (size_t)kPcgBlocks));
        SMH_TRY(ws.alloc(&yt, m * kLdyMax));
        SMH_TRY(ws.alloc(&st, 1));
        const size_t head = offsetof(EgState<T>, ab) + 2 * m * sizeof(T);
        SMH_TRY(run.h_sc.alloc(head, hipHostMallocDefault));
        SMH_TRY(h_yt.alloc(m * kLdyMax * sizeof(T), hipHostMallocDefault));
        const EgState<T> *h_st = (const EgState<T> *)run.h_sc.get();
        T *h_y = (T *)h_yt.get();
        // the set-up: v -> w (scratch), nv, v_0
        SMH_HIP(hipStreamSynchronize(a->stream));
        SMH_HIP(hipMemcpyAsync(w, c.start, n * sizeof(T), hipMemcpyDefault, s));
        hipLaunchKernelGGL((k_eg_init<T>), dim3(1), dim3(1), 0, s, st);
        hipLaunchKernelGGL((k_eg_vv<T>), dim3(grid), dim3(kBlock), 0, s, w, (uint64_t)n, part_ww);
        hipLaunchKernelGGL((k_eg_begin<T>), dim3(1), dim3(kBlock), 0, s, st, part_ww, grid);
        hipLaunchKernelGGL((k_eg_norm<T>), dim3(grid), dim3(kBlock), 0, s, st, w, block[0], ld, vin, (uint64_t)n);
        SMH_HIP(hipGetLastError());
        int cur = 0;
        const dim3 fold_grid((unsigned)m);
        auto body = [&]() -> int {
            T *basis = block[cur];
            SMH_TRY(spmv_enqueue(a, vin, n, w, c.variant, s));
            hipLaunchKernelGGL((k_gs_dots<T>), dim3(grid), dim3(kBlock), 0, s, &st->live, &st->j, basis, ld, w, (uint64_t)n, part);
            hipLaunchKernelGGL((k_gs_fold<T>), fold_grid, dim3(kBlock), 0, s, &st->live, &st->j, st->h1, part, grid);
            hipLaunchKernelGGL((k_gs_update<T, false>), dim3(grid), dim3(kBlock), 0, s, &st->live, &st->j, st->h1, basis, ld, w, (uint64_t)n, part_ww);
            hipLaunchKernelGGL((k_gs_dots<T>), dim3(grid), dim3(kBlock), 0, s, &st->live, &st->j, basis, ld, w, (uint64_t)n, part);
            hipLaunchKernelGGL((k_gs_fold<T>), fold_grid, dim3(kBlock), 0, s, &st->live, &st->j, st->h2, part, grid);
            hipLaunchKernelGGL((k_gs_update<T, true>), dim3(grid), dim3(kBlock), 0, s, &st->live, &st->j, st->h2, basis, ld, w, (uint64_t)n, part_ww);
            hipLaunchKernelGGL((k_eg_step<T>), dim3(1), dim3(kBlock), 0, s, st, part_ww, grid);
            hipLaunchKernelGGL((k_eg_norm<T>), dim3(grid), dim3(kBlock), 0, s, st, w, basis, ld, vin, (uint64_t)n);
            SMH_HIP(hipGetLastError());
            return SMH_OK;
        };
        // Yt of `cols` columns is in h_y (rows of ldy): upload it and rotate block[cur]'s first mc columns
        auto rotate = [&](size_t mc, size_t cols, size_t ldy, bool carry, bool to_mvec) -> int {
            const auto t0 = std::chrono::steady_clock::now();  // (the stream is idle: the cycle's poll has just returned)
            SMH_HIP(hipMemcpyAsync(yt, h_y, mc * ldy * sizeof(T), hipMemcpyHostToDevice, s));
            const unsigned tiles = (unsigned)((cols + kEgRotTile - 1) / kEgRotTile);
            if (to_mvec) {
                const unsigned all = (unsigned)((c.evecs->ld + kEgRotTile - 1) / kEgRotTile);  // (the padding columns' tiles too)
                hipLaunchKernelGGL((k_eg_rotate<T, true>), dim3(grid, all), dim3(kBlock), 0, s, block[cur], ld, (unsigned)mc, yt, (unsigned)ldy,
                                   (unsigned)cols, (T *)c.evecs->d.get(), (uint64_t)c.evecs->ld, (uint64_t)n, all);
            } else {
                hipLaunchKernelGGL((k_eg_rotate<T, false>), dim3(grid, tiles + (carry ? 1u : 0u)), dim3(kBlock), 0, s, block[cur], ld, (unsigned)mc, yt,
                                   (unsigned)ldy, (unsigned)cols, block[cur ^ 1], ld, (uint64_t)n, tiles);
            }
            SMH_HIP(hipGetLastError());
            if (time_rotation) {
                SMH_HIP(hipStreamSynchronize(s));
                t_timing.rotation_ms += ms_since(t0);
                t_timing.rotations += 1;
            }
            return SMH_OK;
        };
        for (;;) {
            for (size_t b = (size_t)host.l; b < m; ++b) SMH_TRY(body());
            SMH_HIP(hipMemcpyAsync(run.h_sc.get(), st, head, hipMemcpyDeviceToHost, s));
            SMH_HIP(hipStreamSynchronize(s));
            products = (size_t)h_st->products;
            breakdown = (int)h_st->breakdown;
            if (breakdown == 2) break;
            const size_t mc = h_st->j;  // the cycle's columns: m, or fewer after breakdown 1
            T alpha[kEgMaxM], beta[kEgMaxM];
            for (size_t j = (size_t)host.l; j < mc; ++j) { alpha[j] = h_st->ab[2 * j]; beta[j] = h_st->ab[2 * j + 1]; }
            const auto t0 = std::chrono::steady_clock::now();
            const bool finite = eg_cycle_end(host, (int)mc, alpha, beta);
            t_timing.host_ms += ms_since(t0);
            t_timing.cycles += 1;
            if (!finite) {
                breakdown = 3;
                break;
            }
            const bool stop = (size_t)host.n_conv == k || restarts == c.restart_max || m == n || breakdown == 1;
            if (stop) {
                kk = k < mc ? k : mc;
                if (c.evecs || c.evecs_host) {
                    const size_t ldy = (k + kEgRotTile - 1) / kEgRotTile * kEgRotTile;
                    eg_rotation(host, (int)mc, (int)kk, beta[mc - 1], h_y, ldy, /*lock*/ false);
                    SMH_TRY(rotate(mc, k, ldy, false, c.evecs != nullptr));
                    if (c.evecs_host)
                        for (size_t i = 0; i < k; ++i)
                            SMH_HIP(hipMemcpyAsync((T *)c.evecs_host + i * n, block[cur ^ 1] + i * (size_t)ld, n * sizeof(T), hipMemcpyDefault, s));
                    SMH_HIP(hipStreamSynchronize(s));
                }
                break;
            }
            const size_t l = k + (m - k) / 2;
            const size_t ldy = (l + kEgRotTile - 1) / kEgRotTile * kEgRotTile;
            eg_rotation(host, (int)mc, (int)l, beta[mc - 1], h_y, ldy, /*lock*/ true);
            SMH_TRY(rotate(mc, l, ldy, /*carry*/ true, false));
            cur ^= 1;
            hipLaunchKernelGGL((k_eg_restart<T>), dim3(1), dim3(1), 0, s, st, (uint32_t)l);
            restarts += 1;
        }
        return SMH_OK;
    }, nullptr, nullptr);
    if (rc != SMH_OK) return rc;
    const bool nothing = breakdown == 2 || breakdown == 3;
    if (!nothing) {
        for (size_t i = 0; i < k; ++i) {
            if (c.evals_out) c.evals_out[i] = i < kk ? host.theta[host.wanted[i]] : std::numeric_limits<double>::quiet_NaN();
            if (c.est_out) c.est_out[i] = i < kk ? host.est[i] : std::numeric_limits<double>::quiet_NaN();
        }
    }
    if (c.n_conv_out) *c.n_conv_out = nothing ? 0 : (size_t)host.n_conv;
    if (c.restarts_out) *c.restarts_out = restarts;
    if (c.products_out) *c.products_out = products;
    if (c.breakdown_out) *c.breakdown_out = breakdown;
    return SMH_OK;
}

// k, ncv and which, after the handles' and the dimensions' checks; *ncv leaves as m
int check_eig_shape(size_t n, size_t k, size_t *ncv, int which) {
    if (k == 0 || k > n) return fail(SMH_ERR_INVALID, "k is %zu: it must be at least 1 and at most the dimension, %zu", k, n);
    if (which != SMH_EIGSH_LARGEST && which != SMH_EIGSH_SMALLEST) return fail(SMH_ERR_INVALID, "which is %d: SMH_EIGSH_LARGEST or SMH_EIGSH_SMALLEST", which);
    size_t m = *ncv;
    if (m == 0) {
        m = 2 * k + 1 > 20 ? 2 * k + 1 : 20;
        if (m > (size_t)kEgMaxM) m = kEgMaxM;
    }
    if (m > n || k + 2 > n) m = n;
    if (m > (size_t)kEgMaxM || (k + 2 <= n && m < k + 2))
        return fail(SMH_ERR_INVALID, "ncv is %zu: after clipping to the dimension it must lie in [k + 2, %d] (0: the default)", *ncv, kEgMaxM);
    *ncv = m;
    return SMH_OK;
}

int eigsh(smh_crs *a, const EigCall &c) {
    if (a->dtype == SMH_F64) return eigsh_t<double>(a, c);
    return eigsh_t<float>(a, c);
}

}  // namespace

// This thread's last smh_eigsh*: the host step's wall time over all its cycle ends, and -- only when the environment variable
// SMH_EIGSH_TIMING is set, which makes the solve wait for every rotation -- the wall time of the rotations (Yt's upload included)
extern "C" int smh_eigsh_last_timing(double *host_step_ms_out, size_t *cycles_out, double *rotation_ms_out, size_t *rotations_out) {
    if (host_step_ms_out) *host_step_ms_out = t_timing.host_ms;
    if (cycles_out) *cycles_out = t_timing.cycles;
    if (rotation_ms_out) *rotation_ms_out = t_timing.rotation_ms;
    if (rotations_out) *rotations_out = t_timing.rotations;
    return SMH_OK;
}

// the statuses are decided here, before any launch
extern "C" int smh_eigsh_vec(smh_crs *m, const smh_vec *start, smh_mvec *evecs, size_t k, size_t ncv, int which, double tol, size_t restart_max,
                             int variant, double *evals_out, double *est_out, size_t *n_conv_out, size_t *restarts_out, size_t *products_out,
                             int *breakdown_out) {
    if (!m || !start) return fail(SMH_ERR_INVALID, "NULL handle");
    if (start->dtype != m->dtype || (evecs && evecs->dtype != m->dtype)) return fail(SMH_ERR_INVALID, "%s", kVecDtype);
    if (m->n_rows != m->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    if (m->n_rows != start->n || (evecs && evecs->n != m->n_rows)) return fail(SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch");
    SMH_TRY(check_eig_shape(m->n_rows, k, &ncv, which));
    if (evecs && evecs->k != k) return fail(SMH_ERR_INVALID, "evecs holds %zu vectors: it must hold k = %zu", evecs->k, k);
    return eigsh(m, {start->d, m->n_rows, k, ncv, which, tol, restart_max, variant, evals_out, nullptr, evecs, est_out, n_conv_out, restarts_out,
                     products_out, breakdown_out});
}

extern "C" int smh_eigsh(smh_crs *m, const void *start_host, size_t start_len, size_t k, size_t ncv, int which, double tol, size_t restart_max,
                         int variant, double *evals_out, void *evecs_host_out, double *est_out, size_t *n_conv_out, size_t *restarts_out,
                         size_t *products_out, int *breakdown_out) {
    if (!m) return fail(SMH_ERR_INVALID, "NULL handle");
    if (m->n_rows != m->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    if (m->n_rows != start_len) return fail(SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch");
    if (start_len && !start_host) return fail(SMH_ERR_INVALID, "NULL host vector");
    SMH_TRY(check_eig_shape(m->n_rows, k, &ncv, which));
    return eigsh(m, {start_host, m->n_rows, k, ncv, which, tol, restart_max, variant, evals_out, evecs_host_out, nullptr, est_out, n_conv_out,
                     restarts_out, products_out, breakdown_out});
}
