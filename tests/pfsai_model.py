"""numpy restatement of GMRES(m) right-preconditioned by a pair of product handles (smh_gmres_fsai_solve*, sparsemat_amd/csrc/gmres.hip)
-- test infrastructure, not product code.  BiCGSTAB with the pair is pbicgstab_model.pbicgstab with the pair's application as its
``precond``: both of a body's applications are formed the same way.

The recurrence is pgmres_model.pgmres's, which this file restates so that the two places M^-1 is applied can be given apart: the
body's u = M^-1 v_j goes through the handles' own kernels, the cycle end's q = M^-1 t through two storage-order products
(SMH_SPMV_SEQ's bits) that run at a cycle end alone.  ``precond`` is the first, ``precond_end`` the second (None: the first again,
and then every output is pgmres_model.pgmres's bit for bit).  ``ends`` of the result lists, per cycle end, the vector t that
``precond_end`` was given.
"""
import numpy as np

import cg_model
import gmres_model as gm
import pgmres_model as pm


def pair(gl, gu, product):
    """v -> G_U (G_L v) with product(off, col, val, x) -> y; gl and gu as (off, col, val)."""
    return lambda v: product(*gu, product(*gl, v))


def pgmres(off, col, val, b, x0, tol, iter_max, restart, precond, precond_end=None, mode="device", product=None):
    """product: where A v comes from (product(v) -> A v in T) -- the initial residual's and every body's."""
    import oracle
    val = np.ascontiguousarray(val)
    T = val.dtype.type
    red = cg_model.Reducer(mode)
    m = restart or gm.DEFAULT_RESTART
    assert 1 <= m <= gm.MAX_RESTART
    mvp = product or (lambda v: oracle.spmv(off, col, val, v))
    at_end = precond_end or precond

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
        rr = rr0 = dot(r, r)
        iters, cycles, breakdown, estimates, basis, ends = 0, 0, 0, [], [], []
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
                w = mvp(precond(basis[j]))
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
            t = basis[0] * y[0]
            for c in range(1, j):
                t = t + basis[c] * y[c]
            ends.append(t.copy())
            x = x + at_end(t)
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
    res = pm.Result(x, iters, T(rr), cycles, breakdown, estimates, basis, T(rr0))
    res.ends = ends
    return res
