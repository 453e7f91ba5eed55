"""numpy restatement of the right-preconditioned BiCGSTAB (smh_bicgstab_precond_solve*, sparsemat_amd/csrc/bicgstab.hip) -- test
infrastructure, not product code.  A M^-1 u = b, x = M^-1 u inside bicgstab_model's recurrence:

    set-up:  unchanged (r = b - A x; r^ = r; p = r; rho = r^.r; rr = r.r; M is not applied to the residual)
    body:    p^ = M^-1 p;  v = A p^;  rv = r^.v;                 rv == 0: breakdown 2 (x untouched)
             alpha = rho / rv;  s = r - v*alpha;  ss = s.s
                                                              sqrt(f64(ss)) < tol: x += p^*alpha; rr = ss; converged
             s^ = M^-1 s;  t = A s^;  ts = t.s;  tt = t.t;       tt == 0: x += p^*alpha; rr = ss; breakdown 3
             omega = ts / tt;  x = (x + p^*alpha) + s^*omega;  r = s - t*omega;  rr = r.r;  rho' = r^.r
             stop test, breakdown 1, beta, p = r + (p - v*omega)*beta: unchanged

Everything else -- the sums (cg_model.Reducer, kind "pcg"), the stop rule, the codes -- is bicgstab_model.bicgstab, which this file
restates rather than calls so that M^-1 stands where the device applies it.  ``precond`` is one of pgmres_model's builders
(``identity``, ``jacobi``, ``sgs``, ``ilu``): a callable v -> M^-1 v in T.  With ``identity`` every number, x included, is
bicgstab_model.bicgstab's; x does not feed back, so from x0 = 0 the bodies, every s.s, every r.r and the code are those of
bicgstab_model.bicgstab(product = A o M^-1).

``wrong``: a deliberately different arithmetic, for the tests that show which variants the bit comparisons can tell apart:
"left" (M^-1 applied to the residual and to A v, omega from the preconditioned vectors: left preconditioning), "x unpreconditioned"
(x takes p and s), "x one application" (x += M^-1 (p*alpha + s*omega)), and for a ``jacobi`` preconditioner "reciprocal"
(v * (1 / d)) and "fma" (the x update's two steps with one rounding each: what contracting them would give).
"""
import math

import numpy as np

import bicgstab_model as bm
import cg_model
import oracle

WRONG = (None, "left", "x unpreconditioned", "x one application", "reciprocal", "fma")


def _fused(x, a, s):
    """x + a * s with ONE rounding (s a scalar of x's type)"""
    wide = np.float64 if x.dtype == np.float32 else np.longdouble
    return (x.astype(wide) + a.astype(wide) * wide(s)).astype(x.dtype)


def pbicgstab(off, col, val, b, x0, tol, iter_max, precond, mode="device", product=None, wrong=None):
    """product: where A v comes from (product(v) -> A v in T; None: oracle.spmv) -- the initial residual's, A p^ and A s^."""
    assert wrong in WRONG
    val = np.ascontiguousarray(val)
    T = val.dtype.type
    red = cg_model.Reducer(mode)
    mvp = product or (lambda v: oracle.spmv(off, col, val, v))
    apply = precond
    if wrong == "reciprocal":
        recip = T(1) / precond.d
        apply = lambda v: v * recip
    left = wrong == "left"

    def dot(a, c):
        return red.dot(a, c, "pcg")

    def axpy(x, a, s):
        return _fused(x, a, s) if wrong == "fma" else x + a * s

    with np.errstate(all="ignore"):
        x = np.array(x0, val.dtype, copy=True)
        b = np.ascontiguousarray(b, val.dtype)
        r = b - mvp(x)
        if left:
            r = apply(r)
        rhat, p = r.copy(), r.copy()
        rho, rr = dot(rhat, r), dot(r, r)
        iters, breakdown, converged, half = 0, 0, False, False
        ss_list, rr_list = [], []
        while iters < iter_max:
            iters += 1
            if left:
                phat, v = p, apply(mvp(p))
            else:
                phat = apply(p)
                v = mvp(phat)
            rv = dot(rhat, v)
            if rv == 0:
                breakdown = 2
                break
            alpha = T(rho / rv)
            s = r - v * alpha
            ss = dot(s, s)
            ss_list.append(ss)
            if wrong == "x unpreconditioned":
                phat = p
            if math.sqrt(float(ss)) < tol:
                x = axpy(x, phat, alpha)
                rr, converged, half = ss, True, True
                break
            if left:
                shat, t = s, apply(mvp(s))
            else:
                shat = apply(s)
                t = mvp(shat)
            if wrong == "x unpreconditioned":
                shat = s
            ts, tt = dot(t, s), dot(t, t)
            if tt == 0:
                x = axpy(x, phat, alpha)
                rr, breakdown = ss, 3
                break
            omega = T(ts / tt)
            if wrong == "x one application":
                x = x + apply(p * alpha + s * omega)
            else:
                x = axpy(axpy(x, phat, alpha), shat, omega)
            r = s - t * omega
            rr, rho_new = dot(r, r), dot(rhat, r)
            rr_list.append(rr)
            if math.sqrt(float(rr)) < tol:
                converged = True
                break
            if rho_new == 0 or omega == 0:
                breakdown = 1
                break
            beta = T(T(rho_new / rho) * T(alpha / omega))
            rho = rho_new
            p = r + (p - v * omega) * beta
        assert x.dtype == r.dtype == val.dtype and type(rr) is T
    return bm.Result(x, iters, T(rr), breakdown, converged, half, ss_list, rr_list, r, p)
