"""numpy restatement of the level-scheduled sparse triangular solve (sparsemat_amd/csrc/trisolve.hip) -- test infrastructure,
not product code.

The triangle of a square CRS matrix: LOWER the stored entries (i, c) with c < i, UPPER those with c > i, plus the diagonal,
which is the FIRST stored (i, i) of a row in storage order (the rule of ``get(i, i)``).  Entries of the other triangle are
ignored.  Everything is carried out with numpy scalars of the matrix's dtype, one rounding per operation:

    s = b[i];  for k in storage order: c = col[k]; if c in the strict triangle: s = s - val[k] * x[c]
    x[i] = s / val[diagpos[i]]   (unit: x[i] = s)

``order`` names the wrong orders a test must be able to tell from the right one: "fma" (s = fma(-val, x, s): one rounding),
"backwards" (the chain from the row's last entry to its first) and "sum_first" (the products summed, subtracted once).
"""
import math

import numpy as np

LOWER, UPPER = "lower", "upper"


def _depends(c, i, uplo):
    return c < i if uplo == LOWER else c > i


def _row_order(n, uplo):
    return range(n) if uplo == LOWER else range(n - 1, -1, -1)


def levels(off, col, uplo):
    """level(i) = 0 if row i has no stored column in the strict triangle, else 1 + max level(c) over them.  Returns
    (level_of_row as uint32 [n], n_levels)."""
    assert uplo in (LOWER, UPPER)
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    n = len(off) - 1
    lev = np.zeros(max(n, 0), np.uint32)
    for i in _row_order(n, uplo):
        c = col[off[i]:off[i + 1]]
        c = c[c < i] if uplo == LOWER else c[c > i]
        lev[i] = 0 if len(c) == 0 else 1 + int(lev[c].max())
    return lev, (int(lev.max()) + 1 if n > 0 else 0)


def diag_positions(off, col):
    """The position in val of each row's first stored (i, i); -1 where there is none."""
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    n = len(off) - 1
    pos = np.full(max(n, 0), -1, np.int64)
    for i in range(n):
        hit = np.flatnonzero(col[off[i]:off[i + 1]] == i)
        if len(hit):
            pos[i] = off[i] + hit[0]
    return pos


def _fma(a, b, c, T):
    """round(a * b + c) in T, exactly: f32 through f64 (the product is exact there and the sum's double rounding is harmless
    for this use: the tests only need a result that differs from two roundings); f64 through fractions."""
    if T is np.float32:
        return T(np.float64(a) * np.float64(b) + np.float64(c))
    from fractions import Fraction
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return T(a * b + c)
    return T(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


class Plan:
    """What ``trisolve`` needs of a pattern, computed once: the levels and, per level, the j-th strict-triangle entry of every
    row that has one.  With it the solve runs level by level on whole arrays -- the same operations on the same operands in the
    same order per row as the row-by-row loop (numpy rounds each array operation once per element), only quicker."""

    def __init__(self, off, col, uplo):
        off = np.asarray(off, np.int64)
        col = np.asarray(col, np.int64)
        n = len(off) - 1
        self.uplo, self.n = uplo, n
        self.level, self.n_levels = levels(off, col, uplo)
        self.pos = diag_positions(off, col)
        deps = [[k for k in range(off[i], off[i + 1]) if _depends(col[k], i, uplo)] for i in range(n)]
        width = max([len(d) for d in deps] + [0])
        K = np.full((n, width), -1, np.int64)
        for i, d in enumerate(deps):
            K[i, :len(d)] = d
        self.steps = []  # per level: (rows, [(rows with a j-th entry, its position)])
        for lv in range(self.n_levels):
            rows = np.flatnonzero(self.level == lv)
            st = []
            for j in range(width):
                sel = K[rows, j] >= 0
                if not sel.any():
                    break
                st.append((rows[sel], K[rows[sel], j]))
            self.steps.append((rows, st))


def trisolve(off, col, val, b, uplo, unit, scale_rhs=False, order="storage", plan=None):
    """x = T^-1 b as smh_crs_trisolve carries it out.  scale_rhs: the right-hand side is b[i] * val[diagpos[i]], rounded once (the
    upper solve of the SGS application).  A row without a diagonal entry is an error unless ``unit`` (and not scale_rhs).
    plan: a ``Plan`` of this pattern and uplo (order "storage" only): the level-by-level form, bit for bit the same."""
    assert uplo in (LOWER, UPPER) and order in ("storage", "fma", "backwards", "sum_first")
    if plan is not None:
        assert order == "storage" and plan.uplo == uplo
        val = np.ascontiguousarray(val)
        col = np.asarray(col, np.int64)
        if (not unit or scale_rhs) and plan.n > 0 and (plan.pos < 0).any():
            raise ValueError("no diagonal entry stored in row %d" % int(np.flatnonzero(plan.pos < 0)[0]))
        x = np.zeros(plan.n, val.dtype)
        s = np.array(b, val.dtype, copy=True)
        with np.errstate(all="ignore"):
            if scale_rhs:
                s = s * val[plan.pos]
            for rows, st in plan.steps:
                for r, k in st:
                    s[r] = s[r] - val[k] * x[col[k]]
                x[rows] = s[rows] if unit else s[rows] / val[plan.pos[rows]]
        return x
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    val = np.ascontiguousarray(val)
    T = val.dtype.type
    n = len(off) - 1
    b = np.ascontiguousarray(b, val.dtype)
    x = np.zeros(max(n, 0), val.dtype)
    pos = diag_positions(off, col)
    if (not unit or scale_rhs) and n > 0 and (pos < 0).any():
        raise ValueError("no diagonal entry stored in row %d" % int(np.flatnonzero(pos < 0)[0]))
    with np.errstate(all="ignore"):
        for i in _row_order(n, uplo):
            s = T(b[i])
            if scale_rhs:
                s = T(s * val[pos[i]])
            ks = [k for k in range(off[i], off[i + 1]) if _depends(col[k], i, uplo)]
            if order == "backwards":
                ks = ks[::-1]
            if order == "sum_first":
                t = T(0)
                for k in ks:
                    t = T(t + T(val[k] * x[col[k]]))
                s = T(s - t)
            else:
                for k in ks:
                    if order == "fma":
                        s = _fma(-val[k], x[col[k]], s, T)
                    else:
                        s = T(s - T(val[k] * x[col[k]]))
            x[i] = s if unit else T(s / val[pos[i]])
    return x


def tri_product(off, col, val, x, uplo, unit):
    """y = T x with the model's own triangle (duplicates each added, the first diagonal entry, the other triangle ignored), in the
    matrix's dtype, storage order, the diagonal term last -- the inverse of ``trisolve`` where every operation is exact."""
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    val = np.ascontiguousarray(val)
    T = val.dtype.type
    n = len(off) - 1
    pos = diag_positions(off, col)
    y = np.zeros(max(n, 0), val.dtype)
    for i in range(n):
        s = T(0)
        for k in range(off[i], off[i + 1]):
            if _depends(col[k], i, uplo):
                s = T(s + T(val[k] * x[col[k]]))
        y[i] = T(s + (x[i] if unit else T(val[pos[i]] * x[i])))
    return y


def dense_triangle(off, col, val, uplo, unit):
    """The triangle as a dense f64 matrix (duplicates added up, the first diagonal entry)."""
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    n = len(off) - 1
    pos = diag_positions(off, col)
    A = np.zeros((n, n))
    for i in range(n):
        for k in range(off[i], off[i + 1]):
            if _depends(col[k], i, uplo):
                A[i, col[k]] += float(val[k])
        A[i, i] = 1.0 if unit else float(val[pos[i]])
    return A


def row_depth(off, col, uplo):
    """Most strict-triangle entries in any row (for error bounds)."""
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    n = len(off) - 1
    return max([sum(1 for k in range(off[i], off[i + 1]) if _depends(col[k], i, uplo)) for i in range(n)] + [0])


# ---- the test matrices ---------------------------------------------------------------------------------------------------
def from_rows(rows, dtype):
    """rows: a list of lists of (column, value) in storage order -> (off, col, val)."""
    off = np.zeros(len(rows) + 1, np.uint32)
    off[1:] = np.cumsum([len(r) for r in rows])
    col = np.array([c for r in rows for c, _ in r], np.uint32)
    val = np.array([v for r in rows for _, v in r], dtype)
    return off, col, val


def awkward(rng, size, dtype):
    """Values whose products and running differences round at every step: odd significands of a few bits more than half the
    format's, so that an FMA, a reversed chain and a sum-first order each move a bit of a chain of two or more terms."""
    T = np.dtype(dtype).type
    bits = 14 if T is np.float32 else 30
    m = rng.integers(2 ** (bits - 1), 2 ** bits, size) * 2 + 1
    return (m.astype(np.float64) / 2.0 ** bits * rng.choice([-1.0, 1.0], size)).astype(dtype)


def chain(n, dtype, seed=0, lower=True):
    """Bidiagonal: row i holds (i, i) and its neighbour (i - 1 for lower): n levels."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        r = [(i, 1.5 + rng.uniform())]
        j = i - 1 if lower else i + 1
        if 0 <= j < n:
            r.insert(0, (j, float(awkward(rng, 1, dtype)[0])))
        rows.append(r)
    return from_rows(rows, dtype)


def dense_lower(n, dtype, seed=0):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        v = awkward(rng, i + 1, dtype) / max(i, 1)
        v[i] = 2.0 + rng.uniform()
        rows.append([(c, float(v[c])) for c in range(i + 1)])
    return from_rows(rows, dtype)


def ragged(max_len, dtype, seed=0):
    """Lower triangle with every strict row length 0 .. max_len (row i has i strict entries for i <= max_len, then a few rows of
    random length), the diagonal entry last in the row."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in list(range(max_len + 1)) + [max_len + 1 + k for k in range(20)]:
        ln = i if i <= max_len else int(rng.integers(0, max_len + 1))
        cols = np.sort(rng.choice(i, ln, replace=False)) if ln else np.zeros(0, np.int64)
        v = awkward(rng, ln, dtype) / max(ln, 1)
        rows.append([(int(c), float(x)) for c, x in zip(cols, v)] + [(i, 2.0 + rng.uniform())])
    return from_rows(rows, dtype)


def messy(n, dtype, seed=0):
    """Unsorted rows with duplicate off-diagonal entries, duplicate diagonals, entries of both triangles and explicit zeros."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        k = int(rng.integers(0, 9))
        cols = rng.integers(0, n, k).tolist()
        if k >= 2:
            cols[1] = cols[0]  # a duplicate
        entries = [(int(c), float(v)) for c, v in zip(cols, awkward(rng, k, dtype) / 4)]
        entries = [(c, v if c != i else 3.0 + rng.uniform()) for c, v in entries]
        entries.insert(int(rng.integers(0, len(entries) + 1)), (i, 2.0 + rng.uniform()))
        if i % 5 == 0:
            entries.append((i, 7.0))  # a second diagonal entry: ignored
        if i % 7 == 3 and i > 0:
            entries.append((i - 1, 0.0))  # a stored zero: a dependency all the same
        rows.append(entries)
    return from_rows(rows, dtype)


def switch_case(R, dtype, seed=0):
    """A chain of 50 rows, then R + 1 independent rows that depend on the chain's last row, then a chain of 50 starting at one of
    them (lower triangular): small levels, one large level, small levels."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(50):
        rows.append(([(i - 1, float(awkward(rng, 1, dtype)[0]))] if i else []) + [(i, 1.5 + rng.uniform())])
    for i in range(50, 50 + R + 1):
        # (magnitudes over many binades: in the transpose, row 49's chain of R + 1 terms then rounds differently from their sum)
        rows.append([(49, float(awkward(rng, 1, dtype)[0]) * 2.0 ** int(rng.integers(-8, 3))), (i, 1.5 + rng.uniform())])
    for i in range(50 + R + 1, 50 + R + 1 + 49):
        rows.append([(i - 1, float(awkward(rng, 1, dtype)[0])), (i, 1.5 + rng.uniform())])
    return from_rows(rows, dtype)


def transpose(off, col, val):
    """(for the UPPER cases: the transposed pattern, rows in ascending column order)"""
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    r = np.repeat(np.arange(n), np.diff(off))
    order = np.lexsort((r, np.asarray(col, np.int64)))
    cnt = np.bincount(np.asarray(col, np.int64), minlength=n)
    o = np.zeros(n + 1, np.uint32)
    o[1:] = np.cumsum(cnt)
    return o, r[order].astype(np.uint32), np.asarray(val)[order]


def reverse(off, col, val):
    """Rows and columns renumbered i -> n - 1 - i, every row's storage order kept: a lower triangle becomes an upper one with the
    same levels."""
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    lens = np.diff(off)[::-1]
    o = np.zeros(n + 1, np.uint32)
    o[1:] = np.cumsum(lens)
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in range(n - 1, -1, -1)]) if n else np.zeros(0, np.int64)
    return o, (n - 1 - np.asarray(col, np.int64)[idx]).astype(np.uint32), np.asarray(val)[idx]
