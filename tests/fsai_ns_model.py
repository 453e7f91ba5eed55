"""numpy restatement of the non-symmetric factorized sparse approximate inverse (smh_crs_fsai_ns, sparsemat_amd/csrc/fsai.hip) -- test
infrastructure, not product code.

M^-1 = G_U G_L ~ A^-1.  The row solve R(C, i) on a CRS matrix C with ascending rows: J = (j_0 < ... < j_(m-1) = i) the stored columns
<= i of row i, B the dense m x m matrix B[p][q] = the stored entry (j_p, j_q) of C or 0 -- the full square.  Every operation is
carried out in the matrix's dtype and rounded once:

    for k = 0 .. m-2:
        for p = k+1 .. m-1:  l_p = B[p][k] / B[k][k]
        for p = k+1 .. m-1, q = k+1 .. m-1:  B[p][q] = B[p][q] - l_p * B[k][q]
        for p = k+1 .. m-1:  B[p][k] = l_p
    y_(m-1) = 1;  for p = m-2 .. 0:  s = 0;  for q = p+1 .. m-1 ascending:  s = s + B[q][p] * y_q;   y_p = -s
    d = B[m-1][m-1]                                  (d * the last row of B^-1 = y)

Row i of G_L is y of R(A, i).  Row i of H is y / d of R(A^T, i), A^T with ascending rows; G_U is the transposition of H as
smh_crs_transpose stores it (fsai_model.transpose; n = 1: a copy).  ``singular`` is the smallest row whose d, in either solve, is
zero or not finite.  A row of either factor with m > MAX_ROW is refused.

``order`` names the wrong variants a test must be able to tell from the right one: "fma" (the update with one rounding), "column"
(B[q][k] in place of B[k][q]: the SPD build's operand), "descending" (the back-substitution sum from q = m-1 down to p+1) and
"recip" (H = y * (1 / d) in place of y / d).

The error bound (``row_bounds``).  The elimination is the LU factorization of B without pivoting: L U = B + E1 with
|E1| <= gamma_m |L| |U| (Higham, Accuracy and Stability, theorem 9.3).  The back substitution solves y^T L = e_m^T on the unit lower
triangle, m - 1 products and sums and a negation per entry: y^T (L + E2) = e_m^T with |E2| <= gamma_m |L|.  The last row of U is
(0, .., 0, d), so y^T (B + E) = d e_m^T with |E| <= gamma_(2m) W, W = |L| |U|.  With x^T B = e_m^T (the exact last row of B^-1):
    y^T / d - x^T = -(y^T / d) E B^-1,   so   |y / d - x|^T <= F^T := gamma_(2m) (|y|^T / |d|) W |B^-1|,
and the division of H adds u |y / d| per entry.  y itself is x~ / x~_m for the x~ of the perturbed system, so to first order
    |y - x / x_m| <= Fy := F / |x_m| + |y| F_m / |x_m|.
Both are taken with a factor 1.1 for the higher-order terms; the f64 solve that stands for "exact" adds the same expression at
f64's unit roundoff (3 m 2^-53 in gamma's place).
"""
import numpy as np

import fsai_model as fm
import ilu_model as im

ORDERS = ("stated", "fma", "column", "descending", "recip")
MAX_ROW = fm.MAX_ROW


def transpose_sorted(off, col, val):
    """A^T with every row's columns ascending (the rows of a matrix that passed check_pattern hold no duplicates)."""
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    n = len(off) - 1
    rows = np.repeat(np.arange(n), np.diff(off))
    order = np.lexsort((rows, col))
    toff = np.zeros(n + 1, np.uint32)
    toff[1:] = np.cumsum(np.bincount(col, minlength=n)) if n else 0
    return toff, rows[order].astype(np.uint32), np.asarray(val)[order]


def square(off, col, val, J):
    """B of a row with columns J: the dense m x m array of the stored (j_p, j_q), both triangles."""
    m = len(J)
    B = np.zeros((m, m), val.dtype)
    for p in range(m):
        k0, k1 = off[J[p]], off[J[p] + 1]
        row = col[k0:k1]
        t = np.searchsorted(row, J)
        hit = (t < len(row)) & (row[np.minimum(t, max(len(row) - 1, 0))] == J) if len(row) else np.zeros(m, bool)
        B[p, np.flatnonzero(hit)] = val[k0 + t[hit]]
    return B


def eliminate(B, order="stated"):
    """The elimination of the definition on a copy of B: U on and above the diagonal, the multipliers below."""
    B = B.copy()
    m = len(B)
    with np.errstate(all="ignore"):
        for k in range(m - 1):
            l = B[k + 1:, k] / B[k, k]
            other = B[k + 1:, k].copy() if order == "column" else B[k, k + 1:]
            sub = B[k + 1:, k + 1:]
            if order == "fma":
                B[k + 1:, k + 1:] = fm._fma(np.broadcast_to(-l[:, None], sub.shape).copy(), np.broadcast_to(other[None, :], sub.shape).copy(), sub)
            else:
                B[k + 1:, k + 1:] = sub - l[:, None] * other[None, :]
            B[k + 1:, k] = l
    return B


def solve_row(B, order="stated"):
    """(y, d, the eliminated B) of the row solve on the square B."""
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
    return y, F[m - 1, m - 1], F


def factor(off, col, val, divide, order="stated", what="row"):
    """(goff, gcol, gval, singular) of one factor of C = (off, col, val): the rows y (divide False) or y / d (True)."""
    goff, gcol = fm.lower_pattern(off, col)
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    val = np.asarray(val)
    T = val.dtype.type
    n = len(off) - 1
    lens = np.diff(goff.astype(np.int64))
    if n and lens.max() > MAX_ROW:
        raise ValueError("%s %d stores more than %d entries" % (what, int(np.flatnonzero(lens > MAX_ROW)[0]), MAX_ROW))
    gval = np.zeros(len(gcol), val.dtype)
    singular = None
    for i in range(n):
        J = gcol[goff[i]:goff[i + 1]].astype(np.int64)
        y, d, _ = solve_row(square(off, col, val, J), order)
        with np.errstate(all="ignore"):
            if divide:
                y = y * T(T(1) / d) if order == "recip" else y / d
        gval[goff[i]:goff[i + 1]] = y
        if not (d != 0 and np.isfinite(d)) and singular is None:
            singular = i
    return goff, gcol, gval, singular


def fsai_ns(off, col, val, order="stated"):
    """(gl, gu, singular): gl and gu as (off, col, val) in the matrix's dtype, gu as the library's transposition stores it."""
    assert order in ORDERS
    im.check_pattern(off, col)
    loff, lcol, lval, sing_l = factor(off, col, val, False, order, "row")
    hoff, hcol, hval, sing_u = factor(*transpose_sorted(off, col, val), True, order, "column")
    both = [s for s in (sing_l, sing_u) if s is not None]
    return (loff, lcol, lval), fm.transpose(hoff, hcol, hval), (min(both) if both else None)


def apply(gl, gu, r, product):
    """z = G_U (G_L r); product(off, col, val, x) -> y."""
    return product(*gu, product(*gl, r))


def dense(off, col, val, dtype=np.float64):
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    A = np.zeros((n, n), dtype)
    A[np.repeat(np.arange(n), np.diff(off)), np.asarray(col, np.int64)] = np.asarray(val).astype(dtype)
    return A


def row_bounds(B):
    """The row solve on B against the derivation above: (y, d, x = the last row of B^-1 by a dense f64 solve, F >= |y / d - x|,
    Fy >= |y - x / x_m|), the bounds as f64 arrays."""
    m = len(B)
    y, d, F = solve_row(B)
    u = 2.0 ** (-24 if B.dtype == np.float32 else -53)
    L = np.tril(F.astype(np.float64), -1) + np.eye(m)
    U = np.triu(F.astype(np.float64))
    W = np.abs(L) @ np.abs(U)
    B64 = B.astype(np.float64)
    e = np.zeros(m)
    e[-1] = 1.0
    x = np.linalg.solve(B64.T, e)
    ya, da = np.abs(y.astype(np.float64)), abs(float(d))
    Fb = 1.1 * ((2 * m * u + 3 * m * 2.0 ** -53) * ((ya / da) @ W @ np.abs(np.linalg.inv(B64))) + u * ya / da)
    Fy = 1.1 * (Fb / abs(x[-1]) + ya * Fb[-1] / abs(x[-1]))
    return y, d, x, Fb, Fy
