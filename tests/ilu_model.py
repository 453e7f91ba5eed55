"""numpy restatement of the incomplete LU factorization without fill (smh_crs_ilu0, sparsemat_amd/csrc/ilu.hip) and of its
application (smh_crs_ilu_apply_vec) -- test infrastructure, not product code.

The pattern is the matrix's own: rows strictly ascending, every (i, i) stored.  w starts as the values; every operation is
carried out in the matrix's dtype and rounded once:

    for i = 0 .. n-1:
      for kk = off[i] .. off[i+1]-1 in storage order, k = col[kk], while k < i:
          w[kk] = w[kk] / w[diagpos[k]]
          for jj = diagpos[k]+1 .. off[k+1]-1  (j = col[jj] > k):
              if row i stores column j at position t:  w[t] = w[t] - w[kk] * w[jj]

Afterwards w holds the unit-lower L on the (i, c) with c < i and U on those with c >= i.  ``order`` names the wrong variants a
test must be able to tell from the right one: "fma" (w[t] = fma(-w[kk], w[jj], w[t]): one rounding), "descending" (the k loop of
a row from its last strict-lower entry to its first) and "div_after" (the updates of a step formed from the undivided w[kk],
w[t] - (w[kk] * w[jj]) / pivot, and the division taken after them).

ILU-PCG is ``sgs_model.sgs_pcg(..., precond=lambda r: ilu_apply(...))``.
"""
import numpy as np

import trisolve_model as tm

ORDERS = ("storage", "fma", "descending", "div_after")


def check_pattern(off, col):
    """The requirements of smh_crs_ilu0 on a pattern; returns the diagonal positions."""
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    n = len(off) - 1
    for i in range(n):
        c = col[off[i]:off[i + 1]]
        if len(c) > 1 and not (np.diff(c) > 0).all():
            raise ValueError("the columns of row %d are not strictly ascending" % i)
    pos = tm.diag_positions(off, col)
    if n > 0 and (pos < 0).any():
        raise ValueError("no diagonal entry stored in row %d" % int(np.flatnonzero(pos < 0)[0]))
    return pos


def ilu0(off, col, val, order="storage", vector=False, counts=False):
    """(w, zero_pivot): the factor's values in the matrix's dtype and the smallest row whose final U(i, i) == 0 (None: none).
    vector: the updates of one (i, k) step as one array operation -- the same operations on the same operands (numpy rounds each
    array operation once per element), only quicker on long pivot rows.  counts: a third result, the number of update terms every
    entry received (d_ij of the error bound)."""
    assert order in ORDERS and not (vector and order == "fma")
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    w = np.array(val, copy=True)
    T = w.dtype.type
    n = len(off) - 1
    pos = check_pattern(off, col)
    d = np.zeros(len(w), np.int64)
    with np.errstate(all="ignore"):
        for i in range(n):
            k0, k1 = off[i], off[i + 1]
            row = col[k0:k1]
            lower = [kk for kk in range(k0, k1) if col[kk] < i]
            if order == "descending":
                lower = lower[::-1]
            for kk in lower:
                k = col[kk]
                piv = w[pos[k]]
                m = w[kk]  # (the undivided value: "div_after" forms its updates from it)
                w[kk] = T(w[kk] / piv)
                # the entries jj of pivot row k behind its diagonal whose column row i stores, and where (t)
                j0, j1 = pos[k] + 1, off[k + 1]
                js = col[j0:j1]
                p = np.searchsorted(row, js)
                hit = (p < len(row)) & (row[np.minimum(p, len(row) - 1)] == js)
                t, jj = k0 + p[hit], j0 + np.flatnonzero(hit)
                d[t] += 1
                if vector:
                    w[t] = w[t] - ((m * w[jj]) / piv if order == "div_after" else w[kk] * w[jj])
                    continue
                for a, b in zip(t, jj):
                    if order == "fma":
                        w[a] = tm._fma(-w[kk], w[b], w[a], T)
                    elif order == "div_after":
                        w[a] = T(w[a] - T(T(m * w[b]) / piv))
                    else:
                        w[a] = T(w[a] - T(w[kk] * w[b]))
    zero = np.flatnonzero(w[pos] == 0) if n > 0 else np.zeros(0, np.int64)
    zp = int(zero[0]) if len(zero) else None
    return (w, zp, d) if counts else (w, zp)


def ilu_apply(off, col, fval, r, plans=None):
    """z = U^-1 L^-1 r on a factor's values.  plans: (Plan LOWER, Plan UPPER) of the pattern (same bits, quicker)."""
    lo, up = plans if plans else (None, None)
    w = tm.trisolve(off, col, fval, r, tm.LOWER, True, plan=lo)
    return tm.trisolve(off, col, fval, w, tm.UPPER, False, plan=up)


def dense_factors(off, col, w):
    """(L, U) of a factor's values as dense f64 matrices (L with its unit diagonal)."""
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    n = len(off) - 1
    L, U = np.eye(n), np.zeros((n, n))
    for i in range(n):
        for k in range(off[i], off[i + 1]):
            if col[k] < i:
                L[i, col[k]] = float(w[k])
            else:
                U[i, col[k]] = float(w[k])
    return L, U


# ---- the test matrices (rows strictly ascending, every diagonal stored) ---------------------------------------------------
def diagonal(n, dtype, seed=0):
    rng = np.random.default_rng(seed)
    return np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), (1.0 + rng.uniform(size=n)).astype(dtype)


def chain(n, dtype, seed=0):
    """Tridiagonal, so that every row has one elimination step with one update: n levels, each of one row."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        r = []
        if i > 0:
            r.append((i - 1, float(tm.awkward(rng, 1, dtype)[0])))
        r.append((i, 2.5 + rng.uniform()))
        if i + 1 < n:
            r.append((i + 1, float(tm.awkward(rng, 1, dtype)[0])))
        rows.append(r)
    return tm.from_rows(rows, dtype)


def dense(n, dtype, seed=0):
    """Fully dense, diagonally dominant: row i has i elimination steps."""
    rng = np.random.default_rng(seed)
    A = tm.awkward(rng, n * n, dtype).reshape(n, n).astype(np.float64)
    A[np.arange(n), np.arange(n)] = n * (1.0 + rng.uniform(size=n))
    return tm.from_rows([[(c, A[i, c]) for c in range(n)] for i in range(n)], dtype)


def ragged(n, dtype, seed=0, period=131, upper=3):
    """Row i has i mod period strict-lower entries, its diagonal and i mod (upper + 1) strict-upper entries (as many as there are
    columns on that side); the diagonal dominates."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        ln = min(i % period, i)
        lo = np.sort(rng.choice(i, ln, replace=False)) if ln else np.zeros(0, np.int64)
        nu = min(i % (upper + 1), n - 1 - i)
        up = np.sort(rng.choice(np.arange(i + 1, n), nu, replace=False)) if nu else np.zeros(0, np.int64)
        v = tm.awkward(rng, ln + nu, dtype) / max(ln + nu, 1)
        rows.append([(int(c), float(x)) for c, x in zip(lo, v[:ln])] + [(i, 2.0 + rng.uniform())] +
                    [(int(c), float(x)) for c, x in zip(up, v[ln:])])
    return tm.from_rows(rows, dtype)


def arrow(n, dtype, first, seed=0):
    """The diagonal plus a dense row and column: the last ones (no fill in the exact LU either; the last diagonal entry takes
    n - 1 updates of random sign, each of the size of a tenth of it), or the first (first=True: every later row then eliminates
    column 0 against a pivot row of n entries, of which it stores one)."""
    rng = np.random.default_rng(seed)
    a, b = tm.awkward(rng, n, dtype), tm.awkward(rng, n, dtype)
    dg = 2.0 + rng.uniform(size=n)
    h = 0 if first else n - 1
    rows = []
    for i in range(n):
        if i == h:
            rows.append([(c, float(dg[c] if c == i else a[c])) for c in range(n)])
        else:
            rows.append(sorted([(h, float(b[i])), (i, float(dg[i]))]))
    return tm.from_rows(rows, dtype)


def random_pattern(n, dtype, per_row=8, seed=0):
    """A non-symmetric pattern of about per_row entries per row with a dominant diagonal."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        c = np.unique(np.append(rng.integers(0, n, per_row - 1), i))
        v = tm.awkward(rng, len(c), dtype)
        rows.append([(int(cc), float(per_row + rng.uniform()) if cc == i else float(x)) for cc, x in zip(c, v)])
    return tm.from_rows(rows, dtype)
