"""numpy restatement of the device-resident restarted GMRES(m) (sparsemat_amd/csrc/gmres.hip) -- test infrastructure, not
product code.  The solver is an extension: the reference has no solver for non-symmetric systems, so this model of the
kernels' own arithmetic is its contract (the recurrence in full: gmres.hip's header).

The recurrence is written once; HOW a reduction is carried out is cg_model's ``mode`` ("sequential", "device", "wide").  Every
other operation is in T with one rounding (a - b*c is a + (-(b*c)): the same bits; numpy's sqrt and division are correctly
rounded), the product A v_j comes from oracle.spmv or from the caller's ``product``, and every reduction of gmres.hip --
v_c.w of both Gram-Schmidt passes, w.w, r.r -- uses solver_tree.hpp's tree on pcg_grid(n): the kind "pcg" of
cg_model.Reducer.  So in "device" mode x, iters, cycles, rr and the breakdown code are the device's bit for bit.

    breakdown   0  none
                1  hn = sqrt(w.w) == 0: the Krylov space is exhausted; x is updated from it (reported also when |g_j| < tol
                   holds in the same body)
                2  the residual a cycle starts from has r.r == 0 (set-up: no body is entered; or after a restart)

Corners the issue left open, decided here and in gmres.hip: v_j = w / hn is formed in EVERY entered body (a cycle's last too:
the rebuilt residual needs it); hn == 0, |g_j| < tol and iters == iter_max all stop the solve and a restart happens only when
none of them holds; `cycles` counts the v_0 formed (1 after a set-up with beta != 0, also when iter_max == 0); the rebuilt r
starts from the product v_0 z_0 (not from 0 + v_0 z_0); z starts as (0, .., 0, g_j) and every transposed rotation is applied
in full (t = c z_i + (-s) z_{i+1}; z_{i+1} = s z_i + c z_{i+1}).

``wrong``: a deliberately different arithmetic, for the tests that show which variants the bit comparisons can tell apart:
"fma" (w - v h with one rounding), "one pass" (no second Gram-Schmidt pass), "descending" (the update over c descending),
"mgs" (modified Gram-Schmidt: every h_c from the w already updated by the columns before it).
"""
import numpy as np

import cg_model
import oracle

DEFAULT_RESTART = 30
MAX_RESTART = 128
TILE = 8  # gmres.hip's kGmTile: columns per load of w in the dots (no bit depends on it)


class Result:
    def __init__(self, x, iterations, rr, cycles, breakdown, estimates, basis, rr0):
        self.x, self.iterations, self.rr, self.cycles, self.breakdown = x, iterations, rr, cycles, breakdown
        self.estimates = list(estimates)  # |f64(g_j)| after every body: what the stop test saw
        self.basis = basis                # v_0 .. v_j of the last cycle (the device keeps them to itself)
        self.rr0 = rr0                    # the initial residual's r.r
        self.r_norm_squared = float(rr)   # what the solver reports: f64(T)


def _fused(w, v, h):
    """w - v*h with ONE rounding (the "fma" variant): exact in f64 for f32 data but for the last rounding, longdouble for f64"""
    wide = np.float64 if w.dtype == np.float32 else np.longdouble
    return (w.astype(wide) - v.astype(wide) * wide(h)).astype(w.dtype)


def gmres(off, col, val, b, x0, tol, iter_max, restart=DEFAULT_RESTART, mode="device", product=None, wrong=None):
    """product: where A v comes from (product(v) -> A v in T; None: oracle.spmv) -- the initial residual's and every body's."""
    assert wrong in (None, "fma", "one pass", "descending", "mgs")
    val = np.ascontiguousarray(val)
    T = val.dtype.type
    red = cg_model.Reducer(mode)
    m = restart or DEFAULT_RESTART
    assert 1 <= m <= MAX_RESTART

    def dot(a, c):
        return red.dot(a, c, "pcg")

    def sub(w, v, h):
        return _fused(w, v, h) if wrong == "fma" else w - v * h

    def gram_schmidt(basis, w):
        order = range(len(basis) - 1, -1, -1) if wrong == "descending" else range(len(basis))
        if wrong == "mgs":
            h = [T(0)] * len(basis)
            for c in order:
                h[c] = dot(basis[c], w)
                w = sub(w, basis[c], h[c])
            return h, w
        h = [dot(v, w) for v in basis]
        for c in order:
            w = sub(w, basis[c], h[c])
        return h, w

    mvp = product or (lambda v: oracle.spmv(off, col, val, v))

    with np.errstate(all="ignore"):
        x = np.array(x0, val.dtype, copy=True)
        b = np.ascontiguousarray(b, val.dtype)
        r = b - mvp(x)
        rr = rr0 = dot(r, r)
        iters, cycles, breakdown, estimates, basis = 0, 0, 0, [], []
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
                w = mvp(basis[j])
                h, w = gram_schmidt(basis, w)
                if wrong != "one pass":
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
            for c in range(j):
                x = x + basis[c] * y[c]
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
    return Result(x, iters, T(rr), cycles, breakdown, estimates, basis, T(rr0))


# ---- the test matrices ---------------------------------------------------------------------------------------------------
def tridiag_skew(n, delta, dtype):
    """tridiag(-1, delta, +1): the skew part dominates, the spectrum lies within delta of the imaginary axis; columns ascending
    within a row.  Returns (off, col, val)."""
    i = np.arange(n, dtype=np.int64)
    cand_col = np.stack([i - 1, i, i + 1], axis=1)
    cand_val = np.broadcast_to(np.array([-1.0, delta, 1.0]), (n, 3))
    keep = np.stack([i > 0, np.ones(n, bool), i < n - 1], axis=1)
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(keep.sum(axis=1), out=off[1:])
    return off, cand_col[keep].astype(np.uint32), cand_val[keep].astype(dtype)


def skew_system(n, delta, dtype):
    """(off, col, val, b, x*) with x* of small integers and b = A x* (exact in both precisions)"""
    off, col, val = tridiag_skew(n, delta, dtype)
    x_star = (np.arange(n) % 7 - 3).astype(dtype)
    return off, col, val, oracle.spmv(off, col, val, x_star), x_star
