"""numpy restatement of the right-preconditioned restarted GMRES(m) (smh_gmres_precond_solve*, sparsemat_amd/csrc/gmres.hip) -- test
infrastructure, not product code.  A M^-1 u = b, x = M^-1 u inside gmres_model's recurrence:

    set-up:     unchanged (r = b - A x; M is not applied to the residual)
    body:       u = M^-1 v_j;  w = A u;  both Gram-Schmidt passes, the step and v_{j+1} = w / hn unchanged
    cycle end:  y unchanged;  t = (..(v_0 y_0 + v_1 y_1) .. + v_{j-1} y_{j-1})   (starts from the product, as r does)
                q = M^-1 t;  x = x + q
                r, rr, the restart: unchanged (rebuilt from the basis; no product)

Everything else -- the sums (cg_model.Reducer, kind "pcg"), the rotations, the stop rule, the codes -- is gmres_model.gmres, which
this file restates rather than calls so that M^-1 stands where the device applies it.  ``precond`` is a callable v -> M^-1 v in T;
the builders ``jacobi``, ``sgs`` and ``ilu`` sit on the models of what the device applies (a division by the first stored (i, i);
sgs_model.sgs_apply; ilu_model.ilu_apply).  x does not feed back into the recurrence, so from x0 = 0 the bodies, cycles,
estimates and rr are those of gmres_model.gmres(product = A o M^-1).

``wrong``: a deliberately different arithmetic, for the tests that show which variants the bit comparisons can tell apart:
"left" (M^-1 applied to the residual and to A v: left preconditioning), "x first" (x accumulated column by column from x, M^-1
applied per term), and for a ``jacobi`` preconditioner "reciprocal" (v * (1 / d)) and "fma" (x + t * (1 / d) with one rounding:
what contracting the cycle end's last operation would give).
"""
import numpy as np

import cg_model
import gmres_model as gm
import ilu_model
import oracle
import sgs_model
import trisolve_model as tm

WRONG = (None, "left", "x first", "reciprocal", "fma")


class Result(gm.Result):
    def __init__(self, *args, x_sums=()):
        super().__init__(*args)
        # per cycle end: (j, |x| before it, sum_c |v_c y_c|, |M^-1 t|) as f64 arrays -- what the bound of the x sums is made of
        self.x_sums = list(x_sums)


# ---- the preconditioners ---------------------------------------------------------------------------------------------------
def identity(v):
    return v.copy()


def jacobi(off, col, val):
    """v -> v / d, d_i the first stored (i, i) (k_pcg_diag); .d is kept for the wrong variants"""
    off64 = np.asarray(off, np.int64)
    n = len(off64) - 1
    rows = np.repeat(np.arange(n), np.diff(off64))
    hits = np.flatnonzero(np.asarray(col, np.int64) == rows)  # (trisolve_model.diag_positions, without its loop over the rows)
    has, first = np.unique(rows[hits], return_index=True)
    assert len(has) == n, "a row without a stored diagonal entry"
    d = np.ascontiguousarray(val)[hits[first]]

    def apply(v):
        with np.errstate(all="ignore"):
            return v / d
    apply.d = d
    return apply


def sgs(off, col, val):
    """smh_crs_sgs_apply_vec's operations on the matrix itself"""
    plans = (tm.Plan(off, col, tm.LOWER), tm.Plan(off, col, tm.UPPER))
    return lambda v: sgs_model.sgs_apply(off, col, val, v, plans)


def ilu(off, col, fval):
    """smh_crs_ilu_apply_vec's operations on a factor's values (ilu_model.ilu0's, or the device's own)"""
    plans = (tm.Plan(off, col, tm.LOWER), tm.Plan(off, col, tm.UPPER))
    return lambda v: ilu_model.ilu_apply(off, col, fval, v, plans)


def _fused_axpy(x, t, s):
    """x + t * s with ONE rounding"""
    wide = np.float64 if x.dtype == np.float32 else np.longdouble
    return (x.astype(wide) + t.astype(wide) * s.astype(wide)).astype(x.dtype)


def pgmres(off, col, val, b, x0, tol, iter_max, restart, precond, mode="device", product=None, wrong=None):
    """product: where A v comes from (product(v) -> A v in T; None: oracle.spmv) -- the initial residual's and every body's."""
    assert wrong in WRONG
    val = np.ascontiguousarray(val)
    T = val.dtype.type
    red = cg_model.Reducer(mode)
    m = restart or gm.DEFAULT_RESTART
    assert 1 <= m <= gm.MAX_RESTART
    mvp = product or (lambda v: oracle.spmv(off, col, val, v))
    apply = precond
    if wrong == "reciprocal":
        recip = T(1) / precond.d
        apply = lambda v: v * recip

    def dot(a, c):
        return red.dot(a, c, "pcg")

    def gram_schmidt(basis, w):
        h = [dot(v, w) for v in basis]
        for c in range(len(basis)):
            w = w - basis[c] * h[c]
        return h, w

    with np.errstate(all="ignore"):
        x = np.array(x0, val.dtype, copy=True)
        b = np.ascontiguousarray(b, val.dtype)
        r = b - mvp(x)
        if wrong == "left":
            r = apply(r)
        rr = rr0 = dot(r, r)
        iters, cycles, breakdown, estimates, basis, x_sums = 0, 0, 0, [], [], []
        while True:
            beta = np.sqrt(rr)
            if beta == 0:
                breakdown = 2
                break
            cycles += 1
            basis, g, cs, sn, R, j = [r / beta], [beta], [], [], [], 0
            if iters >= iter_max:  # (iter_max == 0)
                break
            while True:
                iters += 1
                w = apply(mvp(basis[j])) if wrong == "left" else mvp(apply(basis[j]))
                h, w = gram_schmidt(basis, w)
                h2, w = gram_schmidt(basis, w)
                h = [a + c for a, c in zip(h, h2)]
                hn = np.sqrt(dot(w, w))
                for i in range(j):
                    t = cs[i] * h[i] + sn[i] * h[i + 1]
                    h[i + 1] = (-sn[i]) * h[i] + cs[i] * h[i + 1]
                    h[i] = t
                d = np.sqrt(h[j] * h[j] + hn * hn)
                c, s = h[j] / d, hn / d
                cs.append(c)
                sn.append(s)
                R.append(h[:j] + [c * h[j] + s * hn])  # column j: R[k][i] = R_{i,k}
                g.append((-s) * g[j])
                g[j] = c * g[j]
                j += 1
                basis.append(w.copy() if hn == 0 else w / hn)
                estimates.append(abs(float(g[j])))
                exhausted, conv, last = bool(hn == 0), estimates[-1] < tol, iters == iter_max
                if exhausted or conv or last or j == m:
                    break
            # the cycle end
            y = [T(0)] * j
            for i in range(j - 1, -1, -1):
                a = g[i]
                for k in range(i + 1, j):
                    a = a - R[k][i] * y[k]
                y[i] = a / R[i][i]
            x_before = np.abs(x.astype(np.float64))
            if wrong == "x first":
                for c in range(j):
                    x = x + apply(basis[c] * y[c])
            else:
                t = basis[0] * y[0]
                for c in range(1, j):
                    t = t + basis[c] * y[c]
                if wrong == "left":
                    x = x + t
                elif wrong == "fma":
                    x = _fused_axpy(x, t, T(1) / precond.d)
                else:
                    q = apply(t)
                    x = x + q
                    terms = sum(np.abs(basis[c].astype(np.float64) * np.float64(y[c])) for c in range(j))
                    x_sums.append((j, x_before, terms, np.abs(q.astype(np.float64))))
            z = [T(0)] * j + [g[j]]
            for i in range(j - 1, -1, -1):
                t = cs[i] * z[i] + (-sn[i]) * z[i + 1]
                z[i + 1] = sn[i] * z[i] + cs[i] * z[i + 1]
                z[i] = t
            r = basis[0] * z[0]
            for c in range(1, j + 1):
                r = r + basis[c] * z[c]
            rr = dot(r, r)
            assert all(type(v) is T for v in y + z + g + cs + sn) and r.dtype == x.dtype == val.dtype
            if exhausted:
                breakdown = 1
            if exhausted or conv or last:
                break
    return Result(x, iters, T(rr), cycles, breakdown, estimates, basis, T(rr0), x_sums=x_sums)


# ---- the systems of the issue's table ----------------------------------------------------------------------------------------
def sort_rows(off, col, val):
    """every row by ascending column (the rows hold no duplicates here): what SparseMatCRS.sort_rows leaves"""
    off = np.asarray(off, np.int64)
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order = np.lexsort((np.asarray(col, np.int64), rows))
    return off.astype(np.uint32), np.asarray(col)[order], np.asarray(val)[order]


def scale_rows(off, col, val, seed=7):
    """row i scaled by 2^k_i, k = default_rng(seed).integers(-5, 6, n): exact, and Jacobi undoes it"""
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    k = np.random.default_rng(seed).integers(-5, 6, n)
    return (np.asarray(val) * np.repeat(2.0 ** k, np.diff(off)).astype(np.asarray(val).dtype)), k
