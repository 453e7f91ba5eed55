"""numpy restatement of the symmetric Gauss-Seidel preconditioner and its CG (smh_crs_sgs_apply_vec, smh_pcg_sgs_solve:
sparsemat_amd/csrc/pcg.hip over trisolve.hip) -- test infrastructure, not product code.

M = (D + L) D^-1 (D + U); z = M^-1 r is  w = trisolve(LOWER, r);  u_i = w_i * d_i;  z = trisolve(UPPER, u), each operation
rounded once (tests/trisolve_model.py).  The recurrence is cg_model.pcg's with that z and the same sums: every dot goes through
cg_model.Reducer, kinds "pcg" (r.r, r.z) and "dot" (the unfused p.Ap), so this model is a composition of models that exist.
"""
import math

import numpy as np

import cg_model
import oracle
import trisolve_model as tm


def sgs_apply(off, col, val, r, plans=None):
    """plans: (Plan LOWER, Plan UPPER) of the pattern, to solve level by level (same bits, quicker)."""
    lo, up = plans if plans else (None, None)
    w = tm.trisolve(off, col, val, r, tm.LOWER, False, plan=lo)
    return tm.trisolve(off, col, val, w, tm.UPPER, False, scale_rhs=True, plan=up)


def sgs_pcg(off, col, val, b, x0, tol, iter_max, mode="device", fused=False, product=None, precond=None):
    """smh_pcg_sgs_solve.  product: as in cg_model.pcg.  precond: r -> z (None: sgs_apply; the identity gives plain CG's
    recurrence)."""
    assert not fused or mode == "device"
    val = np.ascontiguousarray(val)
    product = product or (lambda v: oracle.spmv(off, col, val, v))
    if precond is None:
        plans = (tm.Plan(off, col, tm.LOWER), tm.Plan(off, col, tm.UPPER))
        precond = lambda r: sgs_apply(off, col, val, r, plans)
    T = val.dtype.type
    red = cg_model.Reducer(mode)
    with np.errstate(all="ignore"):
        x = np.array(x0, val.dtype, copy=True)
        b = np.ascontiguousarray(b, val.dtype)
        r = b - product(x)
        z = precond(r)
        rr = red.dot(r, r, "pcg")
        rz = red.dot(r, z, "pcg")
        p = z.copy()
        rr0, rr_list, iters = rr, [], 0
        while iters < iter_max:
            iters += 1
            ap = product(p)
            if fused:
                pap = cg_model.fused_pap(p, ap, True)
            else:
                pap = red.one(red.dot(p, ap, "dot"), from_first=True)
            alpha = T(rz / pap)
            r = r - ap * alpha
            rr = red.dot(r, r, "pcg")
            x = x + p * alpha
            rr_list.append(rr)
            if math.sqrt(float(rr)) < tol:
                break
            z = precond(r)
            rz_new = red.dot(r, z, "pcg")
            beta = T(rz_new / rz)
            rz = rz_new
            p = p * beta + z
    return cg_model.Result(x, r, p, iters, rr, rr_list, rr0)


def lap2d(nx, ny, dtype, seed=0, spread=0.0):
    """A five-point operator on an nx x ny grid (vertex (i, j) is row i * ny + j): every edge has a weight w = 10^U(-spread/2,
    spread/2), added to both end points' diagonals and stored as -w; diagonal shift 0.05; columns ascending.  SPD."""
    rng = np.random.default_rng(seed)
    n = nx * ny
    idx = np.arange(n).reshape(nx, ny)
    ea = np.concatenate([idx[:-1, :].ravel(), idx[:, :-1].ravel()])
    eb = np.concatenate([idx[1:, :].ravel(), idx[:, 1:].ravel()])
    w = 10.0 ** rng.uniform(-spread / 2, spread / 2, len(ea)) if spread else np.ones(len(ea))
    diag = np.full(n, 0.05)
    np.add.at(diag, ea, w)
    np.add.at(diag, eb, w)
    r = np.concatenate([ea, eb, np.arange(n)])
    c = np.concatenate([eb, ea, np.arange(n)])
    v = np.concatenate([-w, -w, diag])
    order = np.lexsort((c, r))
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(np.bincount(r, minlength=n))
    return off, c[order].astype(np.uint32), v[order].astype(dtype)


def red_black(nx, ny):
    """perm[new] = old: the stable permutation of the grid's vertices by (i + j) mod 2."""
    i, j = np.divmod(np.arange(nx * ny), ny)
    return np.argsort((i + j) % 2, kind="stable").astype(np.uint32)


def permute_symmetric(off, col, val, perm):
    """P A P^T with perm[new] = old, every row sorted by its new columns (what lap2d's "columns ascending" becomes)."""
    off = np.asarray(off, np.int64)
    perm = np.asarray(perm, np.int64)
    n = len(perm)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    o = np.zeros(n + 1, np.uint32)
    cc, vv = [], []
    for new in range(n):
        k0, k1 = off[perm[new]], off[perm[new] + 1]
        c = inv[np.asarray(col[k0:k1], np.int64)]
        s = np.argsort(c, kind="stable")
        cc.append(c[s])
        vv.append(np.asarray(val[k0:k1])[s])
        o[new + 1] = o[new] + (k1 - k0)
    return o, np.concatenate(cc).astype(np.uint32), np.concatenate(vv).astype(np.asarray(val).dtype)


# the issue's table: (nx, ny, spread, dtype, tol)
TABLE = [(24, 17, 0.0, np.float64, 1e-10), (24, 17, 2.0, np.float64, 1e-10), (40, 33, 1.0, np.float64, 1e-10), (24, 17, 1.0, np.float32, 1e-4)]


def table_case(k, ordering, seed=1):
    """(off, col, val, b) of table row k in the "natural" or the "red_black" ordering; b = A * (a smooth vector + noise)."""
    nx, ny, spread, dtype, tol = TABLE[k]
    off, col, val = lap2d(nx, ny, dtype, seed, spread)
    if ordering == "red_black":
        off, col, val = permute_symmetric(off, col, val, red_black(nx, ny))
    n = nx * ny
    rng = np.random.default_rng(100 + seed)
    b = rng.uniform(-1.0, 1.0, n).astype(dtype)
    return off, col, val, b, tol
