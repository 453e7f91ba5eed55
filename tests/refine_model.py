"""numpy restatement of the mixed-precision iterative refinement (smh_refine_solve*, sparsemat_amd/csrc/refine.hip) and of the
conversion behind smh_crs_cast / smh_vec_cast -- test infrastructure, not product code.

    set-up:  r = b - A x;  rr = r.r;  outer = 0;  inner_iters = 0
    loop:    rr == 0 or sqrt(rr) < tol: code 0;  outer == outer_max: code 1
             e = floor(ilogb(rr) / 2);  r_lo = f32(r * 2^-e);  d_lo = inner solve of A_lo d = r_lo from d = 0
             inner_iters += its bodies;  outer += 1
             x_prev = x;  x = x + f64(d_lo) * 2^e;  r = b - A x;  rr' = r.r
             not (rr' < rr): x = x_prev, code 2, the old rr;  else rr = rr'

Everything is f64 with one rounding per operation but the conversion and the inner solve.  ``product`` (v -> A v in f64) and ``inner``
((r_lo, d_start) -> a result with .x and .iterations, in f32) are callables: the inner solve is one of the existing f32 models (the
builders below), the product the oracle's or the device's own.  r.r is cg_model.device_sum of the rounded squares on pcg's grid from
the first wave's sum (solver_tree.hpp's tree); V = 2 elements per 16-byte vector, 1 when b is not 16-byte aligned.

``wrong``: a deliberately different arithmetic, for the tests that show which variants the bit comparisons can tell apart:
"residual_f32" (b - A x formed in f32), "sequential" (r.r summed left to right), "e_up" (e rounded up), "warm_start" (the inner solve
started from the previous d) and "no_x_prev" (a stalled step is not undone).
"""
import math

import numpy as np

import bicgstab_model as bm
import cg_model
import gmres_model as gm
import oracle
import pbicgstab_model as pb
import pfsai_model as pf
import pgmres_model as pm
import sgs_model

F32, F64 = np.float32, np.float64
WRONG = (None, "residual_f32", "sequential", "e_up", "warm_start", "no_x_prev")
DEFAULT_OUTER_MAX, DEFAULT_INNER_TOL, DEFAULT_INNER_ITER_MAX = 20, 1e-4, 10_000


def cast(a, dtype):
    """numpy's conversion: f64 -> f32 to nearest even, overflow to +-Inf; f32 -> f64 exact"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a).astype(dtype)


def overflow_count(a):
    """finite f64 values that become infinite in f32"""
    a = np.asarray(a, F64)
    return int(np.count_nonzero(np.isfinite(a) & np.isinf(cast(a, F32))))


def scale_exponent(rr, up=False):
    """e = floor(ilogb(rr) / 2) from math.frexp (rr = m 2^ex with m in [0.5, 1): ilogb = ex - 1); a non-finite rr takes 0.
    up: rounded up instead (a wrong variant)."""
    rr = float(rr)
    if not math.isfinite(rr) or rr == 0.0:
        return 0
    l = math.frexp(rr)[1] - 1
    return -((-l) // 2) if up else l // 2


class Result:
    def __init__(self, x, outer, iterations, rr, code, rr_list, inner_list):
        self.x, self.outer, self.iterations, self.rr, self.code = x, outer, iterations, rr, code
        self.rr_list = rr_list        # r.r after the set-up and after every outer step (the refused one of a stall included)
        self.inner_list = inner_list  # the bodies of every inner solve
        self.r_norm_squared = float(rr)


def refine(product, inner, b, x0, tol, outer_max=0, V=2, wrong=None):
    assert wrong in WRONG
    outer_max = outer_max or DEFAULT_OUTER_MAX
    b = np.ascontiguousarray(b, F64)
    n = len(b)
    grid = cg_model.pcg_grid(n)

    def residual(x):
        if wrong == "residual_f32":
            r = (cast(b, F32) - cast(product(x), F32)).astype(F64)
        else:
            r = b - product(x)
        terms = r * r
        rr = cg_model.sequential_sum(terms) if wrong == "sequential" else cg_model.device_sum(terms, grid, V, from_first=True)
        return r, F64(rr)

    with np.errstate(all="ignore"):
        x = np.array(x0, F64, copy=True)
        r, rr = residual(x)
        outer, iters, code, rr_list, inner_list = 0, 0, 0, [rr], []
        d_lo = np.zeros(n, F32)
        while True:
            if rr == 0 or math.sqrt(float(rr)) < tol:
                code = 0
                break
            if outer == outer_max:
                code = 1
                break
            e = scale_exponent(rr, up=wrong == "e_up")
            r_lo = cast(r * F64(math.ldexp(1.0, -e)), F32)
            res = inner(r_lo, d_lo if wrong == "warm_start" else np.zeros(n, F32))
            d_lo = np.asarray(res.x, F32)
            iters += res.iterations
            inner_list.append(res.iterations)
            outer += 1
            x_prev = x
            x = x + d_lo.astype(F64) * F64(math.ldexp(1.0, e))
            r, rr_new = residual(x)
            rr_list.append(rr_new)
            if not (rr_new < rr):
                if wrong != "no_x_prev":
                    x = x_prev
                code = 2
                break
            rr = rr_new
    return Result(x, outer, iters, rr, code, rr_list, inner_list)


# ---- the inner solves: the existing f32 models on (off, col, val32) -----------------------------------------------------------------
def _product(off, col, val, product):
    return product or (lambda v: oracle.spmv(off, col, val, v))


def inner_cg(off, col, val, tol=DEFAULT_INNER_TOL, iter_max=DEFAULT_INNER_ITER_MAX, product=None, fused=False):
    """smh_cg_solve_vec (the workspaces are 16-byte aligned)"""
    assert val.dtype == F32
    return lambda r, d: cg_model.cg(off, col, val, r, d, tol, iter_max, fused=fused, product=_product(off, col, val, product))


def inner_pcg(off, col, val, precond, tol=DEFAULT_INNER_TOL, iter_max=DEFAULT_INNER_ITER_MAX, product=None, fused=False):
    """smh_pcg_sgs_solve_vec / _ilu_ / _fsai_: sgs_model.sgs_pcg with z = precond(r) (None: SGS on the matrix itself)"""
    assert val.dtype == F32
    return lambda r, d: sgs_model.sgs_pcg(off, col, val, r, d, tol, iter_max, fused=fused, product=_product(off, col, val, product), precond=precond)


def inner_bicgstab(off, col, val, precond=None, tol=DEFAULT_INNER_TOL, iter_max=DEFAULT_INNER_ITER_MAX, product=None):
    """smh_bicgstab_precond_solve_vec (None forwards to the plain solver) / smh_bicgstab_fsai_solve_vec"""
    assert val.dtype == F32
    mvp = _product(off, col, val, product)
    if precond is None:
        return lambda r, d: bm.bicgstab(off, col, val, r, d, tol, iter_max, product=mvp)
    return lambda r, d: pb.pbicgstab(off, col, val, r, d, tol, iter_max, precond, product=mvp)


def inner_gmres(off, col, val, restart, precond=None, precond_end=None, tol=DEFAULT_INNER_TOL, iter_max=DEFAULT_INNER_ITER_MAX, product=None):
    """smh_gmres_precond_solve_vec (None forwards to the plain solver) / smh_gmres_fsai_solve_vec (precond_end: the cycle end's
    application where it is formed another way)"""
    assert val.dtype == F32
    mvp = _product(off, col, val, product)
    if precond is None:
        return lambda r, d: gm.gmres(off, col, val, r, d, tol, iter_max, restart, product=mvp)
    if precond_end is None:
        return lambda r, d: pm.pgmres(off, col, val, r, d, tol, iter_max, restart, precond, product=mvp)
    return lambda r, d: pf.pgmres(off, col, val, r, d, tol, iter_max, restart, precond, precond_end=precond_end, product=mvp)
