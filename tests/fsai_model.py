"""numpy restatement of the factorized sparse approximate inverse (smh_crs_fsai, sparsemat_amd/csrc/fsai.hip) and of its
application (smh_crs_fsai_apply_vec) -- test infrastructure, not product code.

G is lower triangular on the stored (i, c) of A with c <= i (rows strictly ascending, every (i, i) stored: a prefix of each
row).  For row i let J = (j_0 < ... < j_(m-1) = i) be those columns and B the dense lower triangle B[p][q], q <= p: the stored
entry (j_p, j_q) of row j_p, or 0 where none is stored.  Every operation is carried out in the matrix's dtype and rounded once:

    for k = 0 .. m-2:
        for p = k+1 .. m-1:  l_p = B[p][k] / B[k][k]
        for p = k+1 .. m-1, q = k+1 .. p:  B[p][q] = B[p][q] - l_p * B[q][k]      (B[q][k]: the value before its division)
        for p = k+1 .. m-1:  B[p][k] = l_p
    y_(m-1) = 1;  for p = m-2 .. 0:  s = 0;  for q = p+1 .. m-1 ascending:  s = s + B[q][p] * y_q;   y_p = -s
    g = 1 / sqrt(B[m-1][m-1]);  G[i, j_p] = y_p * g

not_spd is the smallest row whose last pivot B[m-1][m-1] is not > 0.  A row with m > MAX_ROW is refused.

``order`` names the wrong variants a test must be able to tell from the right one: "fma" (B[p][q] = fma(-l_p, B[q][k], B[p][q]):
one rounding), "descending" (the back-substitution sum from q = m-1 down to p+1), "recip" (l_p = B[p][k] * (1 / B[k][k])),
"div_sqrt" (G = y_p / sqrt(pivot) instead of y_p * g) and "upper" (B[p][q] read from row j_q, column j_p: A's upper triangle).

The error bound (``bounds``).  The elimination is the LDL^T factorization of B without pivoting, so the computed factors satisfy
L D L^T = B + E1 with |E1| <= gamma_(m+1) W, W = |L| |D| |L^T| (Higham, Accuracy and Stability, theorem 10.3 carried over from
R^T R to L D L^T: every entry takes at most m - 1 updates of a product and a difference, and one division).  The right-hand side is
e_m, so the forward solve and the division by D are exact: what is left is the back substitution on the unit upper triangle, m - 1
products and sums and a negation per row, (L^T + E2) y = e_m with |E2| <= gamma_m |L^T|.  Together (B + E) y = d e_m with d the last
pivot and |E| <= gamma_(2m+1) W.  The scaling takes a square root, a division and a product: G_p = y_p / sqrt(d) (1 + theta_3).
  * diag(G A G^T)_i - 1 = (y^T B y (1 + theta_6) - d) / d, and y^T B y = d y_m - y^T E y = d - y^T E y, so with |B| <= W + |E1|
        |diag_i - 1| <= gamma_(2m+7) (|y|^T W |y|) / d                                                      (to first order)
  * against the exact row x / sqrt(x_m), B x = e_m: y / d - x = -B^-1 E y / d, so F = gamma_(2m+1) |B^-1| W |y| / d bounds |y / d -
    x| componentwise; the normalisation by sqrt(x_m) moves every entry by half the relative error of x_m:
        |G_p - x_p / sqrt(x_m)| <= F_p / sqrt(x_m) + |G_p| (F_m / (2 x_m) + gamma_3)
Both are taken with a factor 1.1 for the higher-order terms.

FSAI-PCG is ``sgs_model.sgs_pcg(..., precond=lambda r: fsai_apply(...))``.
"""
import numpy as np

import ilu_model as im
import oracle

ORDERS = ("stated", "fma", "descending", "recip", "div_sqrt", "upper")
MAX_ROW = 128  # kFsaiMaxRow of csrc/fsai.hip


def _fma(a, b, c):
    """round(a * b + c) elementwise, to the last bit almost everywhere (the tests only need a result that differs from two
    roundings): f32 through f64, where the product is exact; f64 through the error-free product (Dekker) and sum (Knuth)."""
    if a.dtype == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    split = 134217729.0  # 2^27 + 1
    p = a * b
    ah = (a * split) - ((a * split) - a)
    bh = (b * split) - ((b * split) - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    t = s - p
    f = (p - (s - t)) + (c - t)
    out = s + (e + f)
    return np.where(np.isfinite(out), out, a * b + c)


def lower_pattern(off, col):
    """(goff, gcol): the stored (i, c) with c <= i -- a prefix of every row, which ilu_model.check_pattern has looked at."""
    im.check_pattern(off, col)
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    n = len(off) - 1
    keep = col <= np.repeat(np.arange(n), np.diff(off))
    goff = np.zeros(n + 1, np.uint32)
    goff[1:] = np.cumsum(np.add.reduceat(keep.astype(np.int64), off[:-1])) if n else 0
    if n and (np.diff(off) == 0).any():  # (reduceat repeats a neighbour for an empty row; check_pattern allows none, but be exact)
        goff[1:] = np.cumsum([keep[off[i]:off[i + 1]].sum() for i in range(n)])
    return goff, col[keep].astype(np.uint32)


def triangle(off, col, val, J, upper=False):
    """B of a row with columns J as a dense m x m array of the matrix's dtype (the strict upper part is 0)."""
    m = len(J)
    B = np.zeros((m, m), val.dtype)
    for p in range(m):
        k0, k1 = off[J[p]], off[J[p] + 1]
        row = col[k0:k1]
        want = J[:p + 1] if not upper else J[p:]
        t = np.searchsorted(row, want)
        hit = (t < len(row)) & (row[np.minimum(t, len(row) - 1)] == want)
        if upper:  # the entry (j_p, j_q) of row j_p with q >= p takes the place of B[q][p]
            B[p + np.flatnonzero(hit), p] = val[k0 + t[hit]]
        else:
            B[p, np.flatnonzero(hit)] = val[k0 + t[hit]]
    return B


def eliminate(B, order="stated"):
    """The elimination of the definition on a copy of B (its lower triangle): unit-lower multipliers below the pivots."""
    B = B.copy()
    T = B.dtype.type
    m = len(B)
    low = np.tril(np.ones((m, m), bool))
    with np.errstate(all="ignore"):
        for k in range(m - 1):
            colk = B[k + 1:, k].copy()
            l = colk * T(T(1) / B[k, k]) if order == "recip" else colk / B[k, k]
            sub = B[k + 1:, k + 1:]
            if order == "fma":
                new = _fma(np.broadcast_to(-l[:, None], sub.shape).copy(), np.broadcast_to(colk[None, :], sub.shape).copy(), sub)
            else:
                new = sub - l[:, None] * colk[None, :]
            B[k + 1:, k + 1:] = np.where(low[k + 1:, k + 1:], new, sub)
            B[k + 1:, k] = l
    return B


def solve_row(B, order="stated"):
    """(the row of G, the last pivot, y) from the triangle B."""
    T = B.dtype.type
    m = len(B)
    F = eliminate(B, order)
    y = np.zeros(m, B.dtype)
    y[m - 1] = T(1)
    with np.errstate(all="ignore"):
        for p in range(m - 2, -1, -1):
            s = T(0)
            for q in (range(m - 1, p, -1) if order == "descending" else range(p + 1, m)):
                s = T(s + T(F[q, p] * y[q]))
            y[p] = -s
        d = F[m - 1, m - 1]
        if order == "div_sqrt":
            g = y / np.sqrt(d)
        else:
            g = y * T(T(1) / np.sqrt(d))
    return g.astype(B.dtype), d, y, F


def fsai(off, col, val, order="stated"):
    """(goff, gcol, gval, not_spd): G in the matrix's dtype and the smallest row whose last pivot is not > 0 (None: none)."""
    assert order in ORDERS
    goff, gcol = lower_pattern(off, col)
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    val = np.asarray(val)
    n = len(off) - 1
    lens = np.diff(goff.astype(np.int64))
    if n and lens.max() > MAX_ROW:
        raise ValueError("row %d stores more than %d entries on or below the diagonal" % (int(np.flatnonzero(lens > MAX_ROW)[0]), MAX_ROW))
    gval = np.zeros(len(gcol), val.dtype)
    not_spd = None
    for i in range(n):
        J = gcol[goff[i]:goff[i + 1]].astype(np.int64)
        g, d, _, _ = solve_row(triangle(off, col, val, J, order == "upper"), order)
        gval[goff[i]:goff[i + 1]] = g
        if not d > 0 and not_spd is None:
            not_spd = i
    return goff, gcol, gval, not_spd


def transpose(goff, gcol, gval):
    """G^T as smh_crs_transpose stores it: the reference's transposition (oracle.transpose: `set(j, i, v)` for every entry in
    storage order, and a push prepends, so a row of G^T holds its columns descending).  n = 1: a copy of G, where the replay of
    one operation would leave an orphan and no row."""
    if len(gcol) <= 1:
        return np.array(goff, np.uint32), np.array(gcol, np.uint32), np.array(gval)
    n_rows, n_cols, off, col, val = oracle.transpose(goff, gcol, gval)[:5]
    assert n_rows == n_cols == len(goff) - 1
    return off, col, val


def fsai_apply(g, gt, r, product):
    """z = G^T (G r); g, gt: (off, col, val); product(off, col, val, x) -> y."""
    return product(*gt, product(*g, r))


def symmetric_dense(off, col, val):
    """The symmetric matrix that A's lower triangle defines, dense f64."""
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    A = np.zeros((n, n))
    r = np.repeat(np.arange(n), np.diff(off))
    c = np.asarray(col, np.int64)
    low = c <= r
    A[r[low], c[low]] = np.asarray(val, np.float64)[low]
    return np.tril(A) + np.tril(A, -1).T


def bounds(off, col, val, goff, gcol, i):
    """Row i against the derivation above: (diag(G A G^T)_i evaluated in extended precision, the bound on its distance from 1, the
    model's row, the exact row by a dense f64 solve, the bound on their distance per entry -- the solve's own error, the same
    expression at f64's unit roundoff, is part of it)."""
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    J = gcol[goff[i]:goff[i + 1]].astype(np.int64)
    m = len(J)
    B = triangle(off, col, np.asarray(val), J)
    g, d, y, F = solve_row(B)
    u = 2.0 ** (-24 if B.dtype == np.float32 else -53)
    L = np.tril(F.astype(np.float64), -1) + np.eye(m)
    W = np.abs(L) @ np.diag(np.abs(np.diag(F).astype(np.float64))) @ np.abs(L.T)
    ya, d = np.abs(y.astype(np.float64)), float(d)
    diag_bound = 1.1 * (2 * m + 7) * u * (ya @ W @ ya) / d
    Bs = np.tril(B.astype(np.float64)) + np.tril(B.astype(np.float64), -1).T
    gl = g.astype(np.longdouble)
    diag = float(gl @ Bs.astype(np.longdouble) @ gl)
    e = np.zeros(m)
    e[-1] = 1.0
    x = np.linalg.solve(Bs, e)
    exact = x / np.sqrt(x[-1])
    Fb = ((2 * m + 1) * u + 3 * m * 2.0 ** -53) * (np.abs(np.linalg.inv(Bs)) @ (W @ ya)) / d
    row_bound = 1.1 * (Fb / np.sqrt(x[-1]) + np.abs(g.astype(np.float64)) * (Fb[-1] / (2 * x[-1]) + 3 * u))
    return diag, diag_bound, g, exact, row_bound
