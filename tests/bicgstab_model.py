"""numpy restatement of the device-resident BiCGSTAB (sparsemat_amd/csrc/bicgstab.hip) -- test infrastructure, not product
code.  The solver is an extension: the reference has no solver for non-symmetric systems, so this model of the kernels' own
arithmetic is its contract.

The recurrence (van der Vorst, unpreconditioned) is written once; HOW a reduction is carried out is cg_model's ``mode``
("sequential", "device", "wide").  Every other operation is in T with one rounding (a - b*c is a + (-(b*c)): the same
bits), the products A p and A s come from oracle.spmv (the SEQ and K1s kernels are bit-exact against it) or from the caller's
``product`` (tests/test_solver_kernels_gpu.py: the device's own product of any kernel family, checked), and every
reduction of bicgstab.hip uses pcg.hip's tree -- cg_model.device_sum(terms, pcg_grid(n), V, from_first=True), the kind
"pcg" of cg_model.Reducer -- so in "device" mode x, the last r.r, the body count and the breakdown code are the device's bit
for bit.

    breakdown   0  none (converged, or iter_max bodies entered)
                1  rho' == 0 or omega == 0 after a full body: beta is undefined; x keeps that body's update
                2  r^.v == 0: alpha is undefined; x is untouched by that body
                3  t.t == 0: omega is undefined; x has taken p*alpha, r.r is s.s
"""
import math

import numpy as np

import cg_model
import oracle


class Result:
    def __init__(self, x, iterations, rr, breakdown, converged, half_step, ss_list=(), rr_list=(), r=None, p=None):
        self.x, self.iterations, self.rr, self.breakdown, self.converged = x, iterations, rr, breakdown, converged
        self.half_step = half_step       # the stop was the half-step one (s.s under tol)
        self.ss_list, self.rr_list = list(ss_list), list(rr_list)  # s.s / r.r of every body that got as far (what the stop tests saw)
        self.r, self.p = r, p            # as the last full step left them (the device keeps them to itself)
        self.r_norm_squared = float(rr)  # what the solver reports: f64(T)


def bicgstab(off, col, val, b, x0, tol, iter_max, mode="device", product=None):
    """product: where A v comes from (product(v) -> A v in T; None: oracle.spmv) -- the initial residual's, A p and A s."""
    val = np.ascontiguousarray(val)
    T = val.dtype.type
    red = cg_model.Reducer(mode)

    def dot(a, c):
        return red.dot(a, c, "pcg")

    mvp = product or (lambda v: oracle.spmv(off, col, val, v))

    with np.errstate(all="ignore"):
        x = np.array(x0, val.dtype, copy=True)
        b = np.ascontiguousarray(b, val.dtype)
        r = b - mvp(x)
        rhat, p = r.copy(), r.copy()
        rho, rr = dot(rhat, r), dot(r, r)
        iters, breakdown, converged, half = 0, 0, False, False
        ss_list, rr_list = [], []
        while iters < iter_max:
            iters += 1
            v = mvp(p)
            rv = dot(rhat, v)
            if rv == 0:
                breakdown = 2
                break
            alpha = T(rho / rv)
            s = r - v * alpha
            ss = dot(s, s)
            ss_list.append(ss)
            if math.sqrt(float(ss)) < tol:
                x = x + p * alpha
                rr, converged, half = ss, True, True
                break
            t = mvp(s)
            ts, tt = dot(t, s), dot(t, t)
            if tt == 0:
                x = x + p * alpha
                rr, breakdown = ss, 3
                break
            omega = T(ts / tt)
            x = (x + p * alpha) + s * omega
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
    return Result(x, iters, T(rr), breakdown, converged, half, ss_list, rr_list, r, p)


# ---- the test matrices ---------------------------------------------------------------------------------------------------
def convdiff2d(g, c, dtype):
    """Five-point convection-diffusion stencil on a g x g grid (row i = y * g + x): diagonal 4 + c, west -1 - c, east -1,
    south -1 - c/2, north -1 + c/2; within a row the columns are stored in that order (neighbours off the grid are left
    out).  Non-symmetric for c != 0.  Returns (off, col, val)."""
    n = g * g
    i = np.arange(n, dtype=np.int64)
    xx, yy = i % g, i // g
    cand_col = np.stack([i, i - 1, i + 1, i - g, i + g], axis=1)
    cand_val = np.broadcast_to(np.array([4 + c, -1 - c, -1.0, -1 - c / 2, -1 + c / 2]), (n, 5))
    keep = np.stack([np.ones(n, bool), xx > 0, xx < g - 1, yy > 0, yy < g - 1], axis=1)
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(keep.sum(axis=1), out=off[1:])
    return off, cand_col[keep].astype(np.uint32), cand_val[keep].astype(dtype)


def tridiag_ns(n, c, dtype, seed=0):
    """Non-symmetric tridiagonal matrix of any n: sub-diagonal -1 - c, diagonal 2 + c + u_i with u uniform in [0, 1),
    super-diagonal -1; columns ascending within a row.  Returns (off, col, val)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    u = rng.uniform(0.0, 1.0, n)
    cand_col = np.stack([i - 1, i, i + 1], axis=1)
    cand_val = np.stack([np.full(n, -1.0 - c), 2.0 + c + u, np.full(n, -1.0)], axis=1)
    keep = np.stack([i > 0, np.ones(n, bool), i < n - 1], axis=1)
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(keep.sum(axis=1), out=off[1:])
    return off, cand_col[keep].astype(np.uint32), cand_val[keep].astype(dtype)


def dense_to_crs(a, dtype):
    """A small dense matrix as CRS, every entry stored (explicit zeros too).  Returns (off, col, val)."""
    a = np.asarray(a, dtype)
    n, m = a.shape
    off = (np.arange(n + 1) * m).astype(np.uint32)
    col = np.tile(np.arange(m, dtype=np.uint32), n)
    return off, col, a.reshape(-1).copy()


def convdiff_system(g, c, dtype):
    """(off, col, val, b, x*) with b = A x*, x* uniform in [-1, 1)"""
    off, col, val = convdiff2d(g, c, dtype)
    x_star = np.random.default_rng(g).uniform(-1, 1, g * g).astype(dtype)
    return off, col, val, oracle.spmv(off, col, val, x_star), x_star


# ---- cases whose result is known exactly: small integers, so every sum is exact in any order ----------------------------------
# (name, A, b, iterations, x, rr, breakdown, converged) from x0 = 0, tol 1e-6, iter_max 10: worked by hand --
#   breakdown 1: r = (-1,-2), rho = 5, v = (6,2), rv = -10, alpha = -1/2, s = (2,-1), ss = 5, t = (-2,-4), ts = 0, tt = 20,
#                omega = 0, x = p*alpha = (1/2, 1), r = s, rr = 5, rho' = r^.r = 0
#   breakdown 3: r = (-3,-3), rho = 18, v = (18,6), rv = -72, alpha = -1/4, s = (3/2,-3/2), ss = 9/2, t = A s = 0, tt = 0
#   breakdown 2: skew: v = A r = (0,-1), r^.v = 0;  b = 0: r = 0, v = 0, r^.v = 0
#   half step:   A = I: v = r, alpha = 1, s = 0
EXACT = [
    ("breakdown 1", [[-2, -2], [-2, 0]], [-1, -2], 1, [0.5, 1.0], 5.0, 1, False),
    ("breakdown 3", [[-3, -3], [-1, -1]], [-3, -3], 1, [0.75, 0.75], 4.5, 3, False),
    ("breakdown 2 (skew)", [[0, 1], [-1, 0]], [1, 0], 1, [0.0, 0.0], 1.0, 2, False),
    ("breakdown 2 (b = 0)", [[2, 1], [0, 3]], [0, 0], 1, [0.0, 0.0], 0.0, 2, False),
    ("half-step stop", np.eye(7).tolist(), [1, 2, 3, 4, 5, 6, 7], 1, [1, 2, 3, 4, 5, 6, 7], 0.0, 0, True),
]
