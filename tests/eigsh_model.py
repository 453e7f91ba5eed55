"""numpy restatement of the device-resident thick-restart Lanczos eigensolver (sparsemat_amd/csrc/eigsh.hip and its host step,
eigsh_host.hpp) -- test infrastructure, not product code.  The solver is an extension: the reference has no eigensolver, so this
model of the kernels' own arithmetic is its contract (the recurrence in full: eigsh.hip's header).

The recurrence is written once; HOW a reduction is carried out is cg_model's ``mode`` ("sequential", "device", "wide").  Every
other operation is in T with one rounding (a - b*c is a + (-(b*c)): the same bits; numpy's sqrt and division are correctly
rounded), the product A v_j comes from oracle.spmv or from the caller's ``product``, and every reduction of eigsh.hip -- v.v of
the set-up, v_c.w of both Gram-Schmidt passes, w.w -- uses solver_tree.hpp's tree on pcg_grid(n): the kind "pcg" of
cg_model.Reducer.  The host step is f64: ``jacobi`` restates eigsh_host.hpp's eg_jacobi operation for operation (numpy's f64
+ - * / sqrt are the C++ ones, nothing is contracted on either side).  So in "device" mode the values, the vectors, the estimates,
n_conv, restarts, products and the breakdown code are the device's bit for bit.

    breakdown   0  none
                1  beta_j = sqrt(w.w) == 0: the Krylov space is exhausted; the min(k, j + 1) pairs that exist are returned
                2  the start vector's norm is zero or not finite: nothing is returned
                3  a non-finite entry of the projected matrix (non-finite data): nothing is returned

Corners the issue left open, decided here and in eigsh.hip: the wanted order is theta ascending for "SA" and that list reversed for
"LA"; "non-finite" is tested on every entry of the projected matrix, before the Jacobi step; breakdowns 2 and 3 return None for
values, vectors and estimates and n_conv = 0; after breakdown 1 with mc < k columns the values and estimates past mc are NaN and the
vectors past mc are the rotation by zero coefficients; v_{j+1} is not formed in a body whose beta_j == 0; n_conv <= k; the stop is
tested after the estimates.

``wrong``: a deliberately different arithmetic, for the tests that show which variants the bit comparisons can tell apart:
"fma" (w - v h with one rounding), "one pass" (no second Gram-Schmidt pass; alpha_j = h1_j), "descending" (the update over c
descending), "rotation descending" (the rotation's sum over c descending), "rotation from zero" (the rotation's sum starts from
0 + v_0 Yt[0, i]: other bits only where that product is -0 and every later one too -- the sign of a zero), "alpha pass 1"
(alpha_j = h1_j alone, both passes still run), "computed coupling" (the arrowhead's s_i replaced by the h_i = h1_i + h2_i that the
first body after a restart computed).
"""
import numpy as np

import cg_model
import oracle

MAX_M = 128
MAX_SWEEPS = 64
LARGEST, SMALLEST = 0, 1
WHICH = {"LA": LARGEST, "SA": SMALLEST}
ROT_TILE = 8   # eigsh.hip's kEgRotTile: output columns per workgroup column of the rotation (no bit depends on it)
WRONG = (None, "fma", "one pass", "descending", "rotation descending", "rotation from zero", "alpha pass 1", "computed coupling")


class Result:
    def __init__(self, values, vectors, estimates, n_conv, restarts, products, breakdown, sweeps, theta_max=None):
        self.values, self.vectors, self.estimates = values, vectors, estimates  # f64 [k], T [k, n], f64 [k]; None: nothing returned
        self.n_conv, self.restarts, self.products, self.breakdown = n_conv, restarts, products, breakdown
        self.sweeps = sweeps  # Jacobi sweeps of every cycle end
        self.theta_max = theta_max  # max_c |theta_c| over the last cycle's Ritz values: what the stop test scaled tol by


def default_tol(dtype):
    """what tol = 0 stands for in the Python surface: 2^10 eps(T)"""
    return 1024.0 * float(np.finfo(dtype).eps)


def clip_ncv(n, k, ncv):
    """m as check_eig_shape leaves it (None: refused)"""
    if k == 0 or k > n:
        return None
    m = ncv or min(MAX_M, max(2 * k + 1, 20))
    if m > n or k + 2 > n:
        m = n
    if m > MAX_M or (k + 2 <= n and m < k + 2):
        return None
    return m


def jacobi(b):
    """eg_jacobi: (theta ascending, ties by index; Y with B = Y diag(theta) Y^T; the number of sweeps) of the symmetric f64 matrix b"""
    b = np.array(b, np.float64)
    m = b.shape[0]
    y = np.eye(m)
    one = np.float64(1.0)
    sweeps = 0
    with np.errstate(all="ignore"):
        while sweeps < MAX_SWEEPS:
            sweeps += 1
            rotations = 0
            for p in range(m - 1):
                for q in range(p + 1, m):
                    a, bpp, bqq = b[p, q], b[p, p], b[q, q]
                    abs_a, abs_p, abs_q = abs(a), abs(bpp), abs(bqq)
                    if abs_p + abs_a == abs_p and abs_q + abs_a == abs_q:
                        b[p, q] = b[q, p] = 0.0
                        continue
                    rotations += 1
                    tau = (bqq - bpp) / (np.float64(2.0) * a)
                    t = one / (abs(tau) + np.sqrt(one + tau * tau))
                    if tau < 0:
                        t = -t
                    c = one / np.sqrt(one + t * t)
                    s = t * c
                    h = t * a
                    x, z = b[:, p].copy(), b[:, q].copy()
                    new_p, new_q = c * x - s * z, s * x + c * z
                    b[:, p] = new_p
                    b[p, :] = new_p
                    b[:, q] = new_q
                    b[q, :] = new_q
                    b[p, p] = bpp - h
                    b[q, q] = bqq + h
                    b[p, q] = b[q, p] = 0.0
                    x, z = y[:, p].copy(), y[:, q].copy()
                    y[:, p] = c * x - s * z
                    y[:, q] = s * x + c * z
            if rotations == 0:
                break
    d = np.diag(b).copy()
    order = np.argsort(d, kind="stable")
    return d[order], y[:, order], sweeps


def projected(theta_l, s_l, alpha, beta, l, mc):
    """the arrowhead + tridiagonal matrix of a cycle, widened to f64"""
    b = np.zeros((mc, mc))
    for i in range(l):
        b[i, i] = float(theta_l[i])
        b[i, l] = b[l, i] = float(s_l[i])
    for j in range(l, mc):
        b[j, j] = float(alpha[j])
        if j + 1 < mc:
            b[j, j + 1] = b[j + 1, j] = float(beta[j])
    return b


def _fused(w, v, h):
    wide = np.float64 if w.dtype == np.float32 else np.longdouble
    return (w.astype(wide) - v.astype(wide) * wide(h)).astype(w.dtype)


def _rotate(basis, yt, wrong):
    """out_i = (..(v_0 Yt[0, i] + v_1 Yt[1, i]) .. + v_{mc-1} Yt[mc-1, i]): starts from the product, ascending"""
    mc, cols = yt.shape
    T = basis[0].dtype.type
    out = []
    for i in range(cols):
        order = list(range(mc))
        if wrong == "rotation descending":
            order.reverse()
        if wrong == "rotation from zero":  # (0 + v_0 Yt[0, i]: the same bits unless the product is -0)
            acc = np.zeros_like(basis[0])
            for c in order:
                acc = acc + basis[c] * T(yt[c, i])
            out.append(acc)
            continue
        acc = basis[order[0]] * T(yt[order[0], i])
        for c in order[1:]:
            acc = acc + basis[c] * T(yt[c, i])
        out.append(acc)
    return out


def eigsh(off, col, val, start, k, ncv=0, which=LARGEST, tol=0.0, restart_max=1000, mode="device", product=None, wrong=None):
    """product: where A v comes from (product(v) -> A v in T; None: oracle.spmv).  tol is used as given."""
    assert wrong in WRONG and which in (LARGEST, SMALLEST)
    val = np.ascontiguousarray(val)
    T = val.dtype.type
    n = len(off) - 1
    m = clip_ncv(n, k, ncv)
    assert m is not None
    red = cg_model.Reducer(mode)
    mvp = product or (lambda v: oracle.spmv(off, col, val, v))

    def dot(a, c):
        return red.dot(a, c, "pcg")

    def sub(w, v, h):
        return _fused(w, v, h) if wrong == "fma" else w - v * h

    def gram_schmidt(basis, w):
        h = [dot(v, w) for v in basis]
        for c in (range(len(basis) - 1, -1, -1) if wrong == "descending" else range(len(basis))):
            w = sub(w, basis[c], h[c])
        return h, w

    with np.errstate(all="ignore"):
        v = np.ascontiguousarray(start, val.dtype)
        nv = np.sqrt(dot(v, v))
        restarts = products = 0
        sweeps = []
        if nv == 0 or not np.isfinite(nv):
            return Result(None, None, None, 0, restarts, products, 2, sweeps)
        basis = [v / nv]
        l = 0
        theta_l, s_l = [], []
        alpha, beta = [T(0)] * m, [T(0)] * m
        while True:
            breakdown = 0
            coupling = None
            j = l
            while j < m:
                products += 1
                w = mvp(basis[j])
                h1, w = gram_schmidt(basis, w)
                if wrong == "one pass":
                    h2 = [T(0)] * len(h1)
                    alpha[j] = h1[j]
                else:
                    h2, w = gram_schmidt(basis, w)
                    alpha[j] = h1[j] if wrong == "alpha pass 1" else h1[j] + h2[j]
                if j == l and l:
                    coupling = [a + c for a, c in zip(h1[:l], h2[:l])]
                beta[j] = np.sqrt(dot(w, w))
                j += 1
                if beta[j - 1] == 0:
                    breakdown = 1
                    break
                basis.append(w / beta[j - 1])
            mc = j
            assert all(type(x) is T for x in alpha[l:mc] + beta[l:mc] + theta_l + s_l)
            s_used = coupling if (wrong == "computed coupling" and coupling is not None) else s_l
            b = projected(theta_l, s_used, alpha, beta, l, mc)
            if not np.isfinite(b).all() or not np.isfinite(float(beta[mc - 1])):
                return Result(None, None, None, 0, restarts, products, 3, sweeps)
            theta, y, sw = jacobi(b)
            sweeps.append(sw)
            wanted = list(range(mc - 1, -1, -1)) if which == LARGEST else list(range(mc))
            thmax = float(np.abs(theta).max())
            est = np.abs(np.float64(beta[mc - 1]) * y[mc - 1, wanted])
            kk = min(k, mc)
            n_conv = 0
            while n_conv < kk and est[n_conv] <= tol * thmax:
                n_conv += 1
            if n_conv == k or restarts == restart_max or m == n or breakdown == 1:
                yt = np.zeros((mc, k), val.dtype)
                yt[:, :kk] = y[:, wanted[:kk]].astype(val.dtype)
                vectors = np.stack(_rotate(basis[:mc], yt, wrong))
                values, estimates = np.full(k, np.nan), np.full(k, np.nan)
                values[:kk] = theta[wanted[:kk]]
                estimates[:kk] = est[:kk]
                assert vectors.dtype == val.dtype
                return Result(values, vectors, estimates, n_conv, restarts, products, breakdown, sweeps, thmax)
            l = k + (m - k) // 2
            yt = y[:, wanted[:l]].astype(val.dtype)
            basis = _rotate(basis[:m], yt, wrong) + [basis[m]]
            theta_l = [T(theta[wanted[i]]) for i in range(l)]
            s_l = [beta[m - 1] * yt[m - 1, i] for i in range(l)]
            restarts += 1


# ---- the test matrices ---------------------------------------------------------------------------------------------------
def crs_from_dense(a, dtype):
    a = np.asarray(a)
    n = a.shape[0]
    off = np.zeros(n + 1, np.uint32)
    cols, vals = [], []
    for i in range(n):
        nz = np.flatnonzero(a[i])
        cols.extend(nz.tolist())
        vals.extend(a[i, nz].tolist())
        off[i + 1] = len(cols)
    return off, np.array(cols, np.uint32), np.array(vals, dtype)


def tridiag_sym(n, dtype, seed=0):
    """tridiag(-1, d_i, -1) with d_i in [2, 4): symmetric, no multiple eigenvalue (an unreduced tridiagonal matrix has none);
    columns ascending within a row.  Returns (off, col, val)."""
    d = 2.0 + 2.0 * np.random.default_rng(seed).random(n)
    i = np.arange(n, dtype=np.int64)
    cand_col = np.stack([i - 1, i, i + 1], axis=1)
    cand_val = np.stack([-np.ones(n), d, -np.ones(n)], axis=1)
    keep = np.stack([i > 0, np.ones(n, bool), i < n - 1], axis=1)
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(keep.sum(axis=1), out=off[1:])
    return off, cand_col[keep].astype(np.uint32), cand_val[keep].astype(dtype)


def grid_operator(nx, ny, dtype, seed=0, shift=0.05):
    """the five-point operator of an nx x ny grid with random edge weights in [0.5, 1.5) plus shift * I: symmetric positive
    definite; (off, col, val) with columns ascending within a row"""
    rng = np.random.default_rng(seed)
    n = nx * ny
    a = np.zeros((n, n))
    for yy in range(ny):
        for xx in range(nx):
            i = yy * nx + xx
            for dx, dy in ((1, 0), (0, 1)):
                if xx + dx < nx and yy + dy < ny:
                    j = (yy + dy) * nx + xx + dx
                    c = 0.5 + rng.random()
                    a[i, j] -= c
                    a[j, i] -= c
                    a[i, i] += c
                    a[j, j] += c
            a[i, i] += shift
    return crs_from_dense(a, dtype)


def dense_of(off, col, val):
    n = len(off) - 1
    a = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(np.asarray(off, np.int64)))
    a[rows, np.asarray(col, np.int64)] = np.asarray(val, np.float64)
    return a


def start_vector(n, dtype, seed=0):
    """what SparseMatCRS.eigsh draws when v0 is None"""
    return np.random.default_rng(seed).standard_normal(n).astype(dtype)
