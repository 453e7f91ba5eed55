// refine.hip -- mixed precision: casting a handle and a vector between f32 and f64 (smh_crs_cast, smh_vec_cast) and iterative
// refinement of an f64 system by the f32 solvers (smh_refine_solve*), gfx950.
//
// EXTENSIONS: the reference has one precision.  Refinement forms the residual of A x = b in f64, solves the correction in f32 with a
// solver the library already has -- through its `_vec` entry point, so its kernels, bits and chains of launches are those -- and adds
// the correction in f64:
//   set-up:  r = b - A x;  rr = r.r
//   loop:    rr == 0 or sqrt(rr) < tol: converged;  outer == outer_max: stop
//            e = floor(ilogb(rr) / 2);  r_lo = (float)(r * 2^-e);  d_lo = 0;  the inner solver on a_lo d_lo = r_lo
//            x_prev = x;  x = x + (double)d_lo * 2^e;  r = b - A x;  rr' = r.r;  not (rr' < rr): x = x_prev, stalled;  rr = rr'
// The scaling is by a power of two, so both products are exact and an outer step rounds each element once going down (the
// conversion) and once going up (the addition); the normalised residual has a norm in [1, 2), which makes the inner solver's absolute
// stop rule a relative one and keeps r_lo . r_lo away from f32 underflow.  Nothing is contracted (-ffp-contract=off and explicitly
// rounded operations).  r.r goes through solver_tree.hpp's tree on pcg's grid: tests/refine_model.py restates the recurrence and
// tests/cg_model.device_sum the sum.
// Device code: the conversion kernel (one pass, 16-byte accesses from an aligned start, a scalar head and tail) and three streaming
// sweeps on solver_tree.hpp's sweep -- the residual with the partials of r.r (and their one-workgroup fold), the scaled conversion
// down, and the save-widen-add that updates x.  The host polls 8 bytes per outer step through a pinned block, as SolveRun does.
#include "crs_forms.hpp"
#include "internal.hpp"
#include "solver_host.hpp"
#include "solver_tree.hpp"

#include <cmath>

using namespace smh;

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr unsigned kCastBlocks = 512;  // 2 blocks per CU, as the solvers' sweeps

// ---- the conversion ---------------------------------------------------------------------------------------------------------------
// f64 -> f32 rounds to nearest even (out-of-range finite values become +-Inf: counted in `over`), f32 -> f64 is exact; NaN stays NaN,
// zeros keep their sign, f32 subnormals are kept (the library's compile mode does not flush them)
__device__ __forceinline__ float cast_down(double v, unsigned &over) {
    const float f = __double2float_rn(v);
    over += (isinf(f) && !isinf(v)) ? 1u : 0u;
    return f;
}

// dst[i] = convert(src[i]) on [0, n): the elements [head, head + 4 nv) by groups of four -- two 16-byte loads for one 16-byte store
// going down, the reverse going up; src + head and dst + head are 16-byte aligned, the host saw to that -- and the head and the tail
// one by one.  overflow (optional, DOWN): += the finite inputs that became infinite, counted per workgroup.
template <bool DOWN>
__global__ void __launch_bounds__(kBlock) k_cast(const void *__restrict__ src_, void *__restrict__ dst_, uint64_t n, uint64_t head, uint64_t nv,
                                                 unsigned long long *__restrict__ overflow) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tail0 = head + 4 * nv;
    unsigned over = 0;
    if constexpr (DOWN) {
        const double *src = (const double *)src_;
        float *dst = (float *)dst_;
        for (uint64_t q = tid; q < nv; q += nthreads) {
            const d2 lo = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(src + head + 4 * q));
            const d2 hi = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(src + head + 4 * q + 2));
            f4 o;
            o[0] = cast_down(lo[0], over); o[1] = cast_down(lo[1], over);
            o[2] = cast_down(hi[0], over); o[3] = cast_down(hi[1], over);
            __builtin_nontemporal_store(o, reinterpret_cast<f4 *>(dst + head + 4 * q));
        }
        for (uint64_t j = tid; j < head + (n - tail0); j += nthreads) {
            const uint64_t i = j < head ? j : tail0 + (j - head);
            dst[i] = cast_down(src[i], over);
        }
    } else {
        const float *src = (const float *)src_;
        double *dst = (double *)dst_;
        for (uint64_t q = tid; q < nv; q += nthreads) {
            const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(src + head + 4 * q));
            d2 lo, hi;
            lo[0] = (double)v[0]; lo[1] = (double)v[1];
            hi[0] = (double)v[2]; hi[1] = (double)v[3];
            __builtin_nontemporal_store(lo, reinterpret_cast<d2 *>(dst + head + 4 * q));
            __builtin_nontemporal_store(hi, reinterpret_cast<d2 *>(dst + head + 4 * q + 2));
        }
        for (uint64_t j = tid; j < head + (n - tail0); j += nthreads) {
            const uint64_t i = j < head ? j : tail0 + (j - head);
            dst[i] = (double)src[i];
        }
    }
    if (DOWN && overflow) {  // (uniform over the grid)
        __shared__ unsigned s_over;
        if (threadIdx.x == 0) s_over = 0;
        __syncthreads();
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) over += (unsigned)__shfl_down((int)over, o, kWave);
        if ((threadIdx.x & (kWave - 1)) == 0 && over) atomicAdd(&s_over, over);
        __syncthreads();
        if (threadIdx.x == 0 && s_over) atomicAdd(overflow, (unsigned long long)s_over);
    }
}

// n values of `from` at src to the other dtype at dst, enqueued on s.  Arrays may start at any 4- / 8-byte boundary: the head runs up
// to the f32 array's first 16-byte boundary, and the groups of four are taken when the f64 array is 16-byte aligned there too.
int launch_cast(int from, const void *src, void *dst, size_t n, unsigned long long *overflow, hipStream_t s) {
    if (n == 0) return SMH_OK;
    const bool down = from == SMH_F64;
    const uintptr_t a32 = (uintptr_t)(down ? dst : src), a64 = (uintptr_t)(down ? src : dst);
    uint64_t head = ((16 - (a32 & 15u)) & 15u) / 4, nv = 0;
    if (head > n) head = n;
    if (((a64 + 8 * head) & 15u) == 0 && ((a32 + 4 * head) & 15u) == 0) nv = (n - head) / 4;
    else head = 0;
    const unsigned grid = grid_for(nv ? nv : n, kCastBlocks);
    if (down) hipLaunchKernelGGL((k_cast<true>), dim3(grid), dim3(kBlock), 0, s, src, dst, (uint64_t)n, head, nv, overflow);
    else hipLaunchKernelGGL((k_cast<false>), dim3(grid), dim3(kBlock), 0, s, src, dst, (uint64_t)n, head, nv, (unsigned long long *)nullptr);
    SMH_HIP(hipGetLastError());
    return SMH_OK;
}

// ---- the three sweeps of an outer step -----------------------------------------------------------------------------------------------
// the pack of at.width f64 values at position `at` of p (the f32 sweep's position: four values are two 16-byte accesses)
template <typename At> struct Wide { typedef double pack __attribute__((ext_vector_type(At::width))); };

template <typename At> __device__ __forceinline__ typename Wide<At>::pack load_wide(const At &at, const double *p) {
    typename Wide<At>::pack v;
    if constexpr (At::width == 4) {
        const d2 lo = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(p + at.i));
        const d2 hi = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(p + at.i + 2));
        v[0] = lo[0]; v[1] = lo[1]; v[2] = hi[0]; v[3] = hi[1];
    } else {
        v[0] = p[at.i];
    }
    return v;
}
template <typename At> __device__ __forceinline__ void store_wide(const At &at, double *p, typename Wide<At>::pack v) {
    if constexpr (At::width == 4) {
        d2 lo, hi;
        lo[0] = v[0]; lo[1] = v[1]; hi[0] = v[2]; hi[1] = v[3];
        __builtin_nontemporal_store(lo, reinterpret_cast<d2 *>(p + at.i));
        __builtin_nontemporal_store(hi, reinterpret_cast<d2 *>(p + at.i + 2));
    } else {
        p[at.i] = v[0];
    }
}

// 1. r = b - ax (one subtraction per element) and part[blockIdx.x] = this workgroup's share of r.r (products rounded, then the tree)
template <SweepWidth W>
__global__ void __launch_bounds__(kBlock)
k_refine_residual(const double *__restrict__ b, const double *__restrict__ ax, double *__restrict__ r, uint64_t n, double *__restrict__ part) {
    double acc = 0.0;
    sweep<double, W>(n, [&](auto at) {
        const auto bv = at.load(b), av = at.load(ax);
        auto rv = bv;
#pragma unroll
        for (int e = 0; e < at.width; ++e) {
            rv[e] = __dsub_rn(bv[e], av[e]);
            acc = p_add(acc, p_mul(rv[e], rv[e]));
        }
        at.store(r, rv);
    });
    block_partial(acc, part);
}
// ... and their fold by one workgroup
__global__ void __launch_bounds__(kBlock) k_refine_fold(const double *__restrict__ part, unsigned n_parts, double *__restrict__ rr) {
    const double v = fold1(part, n_parts);
    if (threadIdx.x == 0) *rr = v;
}

// 2. r_lo = (float)(r * s) with s a power of two (the product is exact: one rounding, the conversion), and d_lo = 0
__global__ void __launch_bounds__(kBlock) k_refine_down(const double *__restrict__ r, double s, float *__restrict__ r_lo, float *__restrict__ d_lo, uint64_t n) {
    sweep<float>(n, [&](auto at) {
        const auto rv = load_wide(at, r);
        typename decltype(at)::pack lo, zero;
#pragma unroll
        for (int e = 0; e < at.width; ++e) {
            lo[e] = __double2float_rn(__dmul_rn(rv[e], s));
            zero[e] = 0.0f;
        }
        at.store(r_lo, lo);
        at.store(d_lo, zero);
    });
}

// 3. x_prev = x;  x = x + (double)d_lo * s with s a power of two (the product is exact: one rounding, the addition)
template <SweepWidth W>
__global__ void __launch_bounds__(kBlock) k_refine_up(double *__restrict__ x, double *__restrict__ x_prev, const float *__restrict__ d_lo, double s, uint64_t n) {
    sweep<float, W>(n, [&](auto at) {
        auto xv = load_wide(at, x);
        const auto dv = at.load(d_lo);
        store_wide(at, x_prev, xv);
#pragma unroll
        for (int e = 0; e < at.width; ++e) xv[e] = __dadd_rn(xv[e], __dmul_rn((double)dv[e], s));
        store_wide(at, x, xv);
    });
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// ---- the driver -----------------------------------------------------------------------------------------------------------------------
struct RefineCall {
    smh_crs *a, *a_lo;
    int inner, precond;
    smh_crs *f_lo, *f2_lo;
    const double *b;  // device, n
    double *x;        // device, n: in the start, out the result
    double tol;
    size_t outer_max;
    double inner_tol;
    size_t inner_iter_max, restart;
    int variant, variant_lo;
    size_t check_every;
    size_t *outer_out, *inner_iters_out;
    double *rr_out;
    int *code_out;
};

// the inner solver on a_lo d = r through its `_vec` entry point (the table of the header); *bodies: the bodies it entered
int inner_solve(const RefineCall &c, const smh_vec *r, smh_vec *d, size_t *bodies) {
    double rr = 0.0;
    size_t cycles = 0;
    int brk = 0;  // (a breakdown is not an error: d is used, and the outer test decides)
    const bool fsai = c.precond == SMH_PRECOND_FSAI;
    switch (c.inner) {
        case SMH_INNER_CG:
            if (fsai) return smh_pcg_fsai_solve_vec(c.a_lo, c.f_lo, c.f2_lo, r, d, c.inner_tol, c.inner_iter_max, c.variant_lo, c.check_every, bodies, &rr);
            if (c.precond == SMH_PRECOND_ILU) return smh_pcg_ilu_solve_vec(c.a_lo, c.f_lo, r, d, c.inner_tol, c.inner_iter_max, c.variant_lo, c.check_every, bodies, &rr);
            if (c.precond == SMH_PRECOND_SGS) return smh_pcg_sgs_solve_vec(c.a_lo, r, d, c.inner_tol, c.inner_iter_max, c.variant_lo, c.check_every, bodies, &rr);
            return smh_cg_solve_vec(c.a_lo, r, d, c.inner_tol, c.inner_iter_max, c.variant_lo, c.check_every, bodies, &rr);
        case SMH_INNER_BICGSTAB:
            if (fsai) return smh_bicgstab_fsai_solve_vec(c.a_lo, c.f_lo, c.f2_lo, r, d, c.inner_tol, c.inner_iter_max, c.variant_lo, c.check_every, bodies, &rr, &brk);
            return smh_bicgstab_precond_solve_vec(c.a_lo, c.precond, c.f_lo, r, d, c.inner_tol, c.inner_iter_max, c.variant_lo, c.check_every, bodies, &rr, &brk);
        default:
            if (fsai) return smh_gmres_fsai_solve_vec(c.a_lo, c.f_lo, c.f2_lo, r, d, c.inner_tol, c.inner_iter_max, c.restart, c.variant_lo, c.check_every, bodies, &rr, &cycles, &brk);
            return smh_gmres_precond_solve_vec(c.a_lo, c.precond, c.f_lo, r, d, c.inner_tol, c.inner_iter_max, c.restart, c.variant_lo, c.check_every, bodies, &rr, &cycles, &brk);
    }
}

// (the checks have passed)
int refine(const RefineCall &c) {
    const size_t n = c.a->n_rows;
    SolveRun run;
    size_t outer = 0, inner_iters = 0;
    int code = 0;
    const int rc = run.run([&]() -> int {
        SMH_TRY(run.own_stream());
        const hipStream_t s = run.s;
        Scratch &ws = run.ws;
        double *r = nullptr, *ax = nullptr, *x_prev = nullptr, *part = nullptr;
        float *r_lo = nullptr, *d_lo = nullptr;
        SMH_TRY(ws.alloc(&r, n)); SMH_TRY(ws.alloc(&ax, n)); SMH_TRY(ws.alloc(&x_prev, n));
        SMH_TRY(ws.alloc(&r_lo, n)); SMH_TRY(ws.alloc(&d_lo, n));
        SMH_TRY(ws.alloc(&part, (size_t)kPcgBlocks + 1));
        SMH_TRY(run.h_sc.alloc(sizeof(double), hipHostMallocDefault));
        double *d_rr = part + kPcgBlocks;
        const unsigned grid = pcg_grid(n);
        smh_vec r_vec, d_vec;  // (borrowed: the workspaces are the run's)
        r_vec.dtype = d_vec.dtype = SMH_F32;
        r_vec.device = d_vec.device = c.a_lo->device;
        r_vec.n = d_vec.n = n;
        r_vec.d = r_lo; d_vec.d = d_lo;
        r_vec.owns = d_vec.owns = false;
        // r = b - A x and rr = r.r; the one host round trip of an outer step
        auto residual = [&](double *rr_host) -> int {
            SMH_TRY(spmv_enqueue(c.a, c.x, n, ax, c.variant, s));
            if (aligned16(c.b)) hipLaunchKernelGGL((k_refine_residual<kBy16Bytes>), dim3(grid), dim3(kBlock), 0, s, c.b, ax, r, (uint64_t)n, part);
            else hipLaunchKernelGGL((k_refine_residual<kByElement>), dim3(grid), dim3(kBlock), 0, s, c.b, ax, r, (uint64_t)n, part);
            hipLaunchKernelGGL(k_refine_fold, dim3(1), dim3(kBlock), 0, s, part, grid, d_rr);
            SMH_HIP(hipGetLastError());
            SMH_HIP(hipMemcpyAsync(run.h_sc.get(), d_rr, sizeof(double), hipMemcpyDeviceToHost, s));
            SMH_HIP(hipStreamSynchronize(s));
            *rr_host = *(const double *)run.h_sc.get();
            return SMH_OK;
        };
        SMH_HIP(hipStreamSynchronize(c.a->stream));  // (the matrix is read on another stream than the one that may have written it)
        SMH_HIP(hipStreamSynchronize(c.a_lo->stream));
        double rr = 0.0;
        SMH_TRY(residual(&rr));
        for (;;) {
            if (rr == 0.0 || std::sqrt(rr) < c.tol) { code = 0; break; }
            if (outer == c.outer_max) { code = 1; break; }
            // |r 2^-e|^2 in [1, 4); a non-finite rr takes e = 0 and ends in the stall below
            int e = 0;
            if (std::isfinite(rr)) {
                const int l = std::ilogb(rr);
                e = l >= 0 ? l / 2 : -((-l + 1) / 2);
            }
            hipLaunchKernelGGL(k_refine_down, dim3(grid), dim3(kBlock), 0, s, r, std::ldexp(1.0, -e), r_lo, d_lo, (uint64_t)n);
            SMH_HIP(hipGetLastError());
            SMH_HIP(hipStreamSynchronize(s));  // (the inner solve runs on a stream of its own)
            size_t bodies = 0;
            SMH_TRY(inner_solve(c, &r_vec, &d_vec, &bodies));  // (drained when it returns)
            inner_iters += bodies;
            outer += 1;
            if (aligned16(c.x)) hipLaunchKernelGGL((k_refine_up<kBy16Bytes>), dim3(grid), dim3(kBlock), 0, s, c.x, x_prev, d_lo, std::ldexp(1.0, e), (uint64_t)n);
            else hipLaunchKernelGGL((k_refine_up<kByElement>), dim3(grid), dim3(kBlock), 0, s, c.x, x_prev, d_lo, std::ldexp(1.0, e), (uint64_t)n);
            SMH_HIP(hipGetLastError());
            double rr_new = 0.0;
            SMH_TRY(residual(&rr_new));
            if (!(rr_new < rr)) {  // stalled (covers NaN): the better iterate comes back, with its rr
                if (n) SMH_HIP(hipMemcpyAsync(c.x, x_prev, n * sizeof(double), hipMemcpyDeviceToDevice, s));
                SMH_HIP(hipStreamSynchronize(s));
                code = 2;
                break;
            }
            rr = rr_new;
        }
        run.rr = rr;
        return SMH_OK;
    }, nullptr, c.rr_out);
    if (rc != SMH_OK) return rc;
    if (c.outer_out) *c.outer_out = outer;
    if (c.inner_iters_out) *c.inner_iters_out = inner_iters;
    if (c.code_out) *c.code_out = code;
    return SMH_OK;
}

// What both entry points decide about the handles and the choice of solver, before any launch, in the header's order; b_len / x_len:
// the vectors' dims.  restart: 0 becomes the default.
int check_refine(const smh_crs *a, const smh_crs *a_lo, int inner, int precond, const smh_crs *f_lo, const smh_crs *f2_lo, size_t b_len, size_t x_len,
                 size_t *restart) {
    if (inner != SMH_INNER_CG && inner != SMH_INNER_BICGSTAB && inner != SMH_INNER_GMRES)
        return fail(SMH_ERR_INVALID, "refine: inner is %d: it must be SMH_INNER_CG, SMH_INNER_BICGSTAB or SMH_INNER_GMRES", inner);
    if (precond != SMH_PRECOND_NONE && precond != SMH_PRECOND_JACOBI && precond != SMH_PRECOND_SGS && precond != SMH_PRECOND_ILU && precond != SMH_PRECOND_FSAI)
        return fail(SMH_ERR_INVALID, "refine: precond is %d: it must be SMH_PRECOND_NONE, _JACOBI, _SGS, _ILU or _FSAI", precond);
    if (inner == SMH_INNER_CG && precond == SMH_PRECOND_JACOBI)
        return fail(SMH_ERR_INVALID, "refine: the Jacobi-preconditioned CG has no device-vector form; take SMH_INNER_BICGSTAB or another preconditioner");
    const int takes = precond == SMH_PRECOND_FSAI ? 2 : precond == SMH_PRECOND_ILU ? 1 : 0;
    if ((takes >= 1) != (f_lo != nullptr) || (takes == 2) != (f2_lo != nullptr))
        return fail(SMH_ERR_INVALID, "refine: this preconditioner takes %d factor handle%s (ILU: f_lo; FSAI: f_lo and f2_lo; the others none)", takes,
                    takes == 1 ? "" : "s");
    if (a_lo->n_rows != a->n_rows || a_lo->n_cols != a->n_cols) return fail(SMH_ERR_DIM_MISMATCH, "refine: a_lo's dimensions differ from a's");
    if (a_lo->device != a->device) return fail(SMH_ERR_INVALID, "refine: a_lo and a live on different devices");
    if (a->n_rows != a->n_cols) return fail(SMH_ERR_NOT_SQUARE, "Matrix is not symmetric");
    if (a->n_rows != b_len || a->n_rows != x_len) return fail(SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch");
    return check_solve_restart(restart, 30, 128);
}

int check_dtypes(const smh_crs *a, const smh_crs *a_lo) {
    if (a->dtype != SMH_F64) return fail(SMH_ERR_INVALID, "refine: a must be an f64 handle");
    if (a_lo->dtype != SMH_F32) return fail(SMH_ERR_INVALID, "refine: a_lo must be an f32 handle (smh_crs_cast(a, SMH_F32))");
    return SMH_OK;
}

void defaults(size_t *outer_max, double *inner_tol, size_t *inner_iter_max) {
    if (*outer_max == 0) *outer_max = 20;
    if (*inner_tol == 0.0) *inner_tol = 1e-4;
    if (*inner_iter_max == 0) *inner_iter_max = 10000;
}

}  // namespace

// ---- the entry points -----------------------------------------------------------------------------------------------------------------
extern "C" int smh_crs_cast(const smh_crs *a, smh_dtype dtype, smh_crs **out, size_t *overflow_out) {
    if (!a || !out) return fail(SMH_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (overflow_out) *overflow_out = 0;
    if (dtype != SMH_F32 && dtype != SMH_F64) return fail(SMH_ERR_INVALID, "dtype must be SMH_F32 or SMH_F64");
    if ((int)dtype == a->dtype) return smh_crs_clone(a, out);
    SMH_HIP(hipStreamSynchronize(a->stream));
    const size_t vs = dtype_size(dtype);
    CrsArrays arrays;
    SMH_TRY(arrays.alloc(a->n_rows, a->nnz, vs));
    SMH_HIP(hipMemcpy(arrays.off, a->d_off, (a->n_rows + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    if (a->nnz) SMH_HIP(hipMemcpy(arrays.col, a->d_col, a->nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    SMH_TRY(arrays.zero_padding(a->nnz, vs, a->stream));
    unsigned long long over = 0;
    {
        Scratch scr;
        unsigned long long *d_over = nullptr;
        SMH_TRY(scr.alloc(&d_over, 1));
        SMH_HIP(hipMemsetAsync(d_over, 0, sizeof *d_over, a->stream));
        const int rc = launch_cast(a->dtype, a->d_val, arrays.val, a->nnz, d_over, a->stream);
        if (rc == SMH_OK) (void)hipMemcpyAsync(&over, d_over, sizeof over, hipMemcpyDeviceToHost, a->stream);
        const hipError_t e = hipStreamSynchronize(a->stream);  // (before the counter goes back to the pool)
        SMH_TRY(rc);
        SMH_HIP(e);
    }
    SMH_TRY(wrap_arrays(dtype, a, a->n_rows, a->n_cols, a->nnz, arrays, 0, out));
    (*out)->orphans = a->orphans;
    (*out)->has_first_op = a->has_first_op;
    (*out)->first_row = a->first_row;
    (*out)->first_col = a->first_col;
    if (a->dtype == SMH_F64) {  // the folded value of a one-operation replay, in the new dtype's bits
        double v;
        memcpy(&v, &a->first_val_bits, sizeof v);
        const float f = (float)v;
        memcpy(&(*out)->first_val_bits, &f, sizeof f);
    } else {
        float f;
        memcpy(&f, &a->first_val_bits, sizeof f);
        const double v = (double)f;
        memcpy(&(*out)->first_val_bits, &v, sizeof v);
    }
    if (overflow_out) *overflow_out = (size_t)over;
    return SMH_OK;
}

extern "C" int smh_vec_cast(const smh_vec *src, smh_vec *dst) {
    if (!src || !dst) return fail(SMH_ERR_INVALID, "NULL vector handle");
    if (src->n != dst->n) return fail(SMH_ERR_DIM_MISMATCH, "Dimension mismatch");
    if (src->dtype == dst->dtype) return smh_vec_copy(dst, src);
    const char *ps = (const char *)src->d, *pd = (const char *)dst->d;
    if (src->n && ps < pd + dst->n * dtype_size(dst->dtype) && pd < ps + src->n * dtype_size(src->dtype))
        return fail(SMH_ERR_INVALID, "smh_vec_cast: src and dst share storage");
    SMH_TRY(launch_cast(src->dtype, src->d, dst->d, src->n, nullptr, nullptr));
    SMH_HIP(hipStreamSynchronize(nullptr));
    return SMH_OK;
}

extern "C" int smh_refine_solve_vec(smh_crs *a, smh_crs *a_lo, int inner, int precond, smh_crs *f_lo, smh_crs *f2_lo, const smh_vec *b, smh_vec *x,
                                    double tol, size_t outer_max, double inner_tol, size_t inner_iter_max, size_t restart, int variant, int variant_lo,
                                    size_t check_every, size_t *outer_out, size_t *inner_iters_out, double *rr_out, int *code_out) {
    if (!a || !a_lo || !b || !x) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(check_dtypes(a, a_lo));
    if (b->dtype != SMH_F64 || x->dtype != SMH_F64) return fail(SMH_ERR_INVALID, "refine: b and x must be f64 vectors");
    if (same_storage(b, x)) return fail(SMH_ERR_INVALID, "b and x are the same storage");
    SMH_TRY(check_refine(a, a_lo, inner, precond, f_lo, f2_lo, b->n, x->n, &restart));
    defaults(&outer_max, &inner_tol, &inner_iter_max);
    return refine({a, a_lo, inner, precond, f_lo, f2_lo, (const double *)b->d, (double *)x->d, tol, outer_max, inner_tol, inner_iter_max, restart, variant,
                   variant_lo, check_every, outer_out, inner_iters_out, rr_out, code_out});
}

extern "C" int smh_refine_solve(smh_crs *a, smh_crs *a_lo, int inner, int precond, smh_crs *f_lo, smh_crs *f2_lo, const void *b_host, size_t b_len,
                                void *x_host_inout, size_t x_len, double tol, size_t outer_max, double inner_tol, size_t inner_iter_max, size_t restart,
                                int variant, int variant_lo, size_t check_every, size_t *outer_out, size_t *inner_iters_out, double *rr_out,
                                int *code_out) {
    if (!a || !a_lo) return fail(SMH_ERR_INVALID, "NULL handle");
    SMH_TRY(check_dtypes(a, a_lo));
    if ((b_len && !b_host) || (x_len && !x_host_inout)) return fail(SMH_ERR_INVALID, "NULL host vector");
    if (b_len && b_host == x_host_inout) return fail(SMH_ERR_INVALID, "b and x are the same storage");
    SMH_TRY(check_refine(a, a_lo, inner, precond, f_lo, f2_lo, b_len, x_len, &restart));
    defaults(&outer_max, &inner_tol, &inner_iter_max);
    const size_t n = a->n_rows;
    Scratch stage;
    double *d_b = nullptr, *d_x = nullptr;
    SMH_TRY(stage.alloc(&d_b, n));
    SMH_TRY(stage.alloc(&d_x, n));
    if (n) {
        SMH_HIP(hipMemcpy(d_b, b_host, n * sizeof(double), hipMemcpyHostToDevice));
        SMH_HIP(hipMemcpy(d_x, x_host_inout, n * sizeof(double), hipMemcpyHostToDevice));
    }
    SMH_TRY(refine({a, a_lo, inner, precond, f_lo, f2_lo, d_b, d_x, tol, outer_max, inner_tol, inner_iter_max, restart, variant, variant_lo, check_every,
                    outer_out, inner_iters_out, rr_out, code_out}));
    if (n) SMH_HIP(hipMemcpy(x_host_inout, d_x, n * sizeof(double), hipMemcpyDeviceToHost));
    return SMH_OK;
}
