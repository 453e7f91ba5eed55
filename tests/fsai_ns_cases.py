"""The matrices of the non-symmetric FSAI tests, shared by tests/test_fsai_ns_model.py (CPU: the bounds, and every case moves a bit
under each wrong variant it can tell apart) and tests/test_fsai_ns_gpu.py (the device equals the model bit for bit on the same cases)."""
import numpy as np

import bicgstab_model as bm
import fsai_ns_model as nm
import pgmres_model as pm
import trisolve_model as tm

MAX_ROW = nm.MAX_ROW  # kFsaiMaxRow of csrc/fsai.hip: a row of either factor with more entries is refused
SLICE = 16            # kFsaiNsSlice: a group of L lanes holds a square of at most SLICE * L values in the LDS
LANES = (1, 2, 4, 8, 16, 32, 64)


def fit(lanes):
    """The longest row (m entries) whose square of m * m values fits the slice of `lanes` lanes: 4, 5, 8, 11, 16, 22, 32.  A longer
    one is a workgroup's, with the square in global scratch."""
    m = 1
    while (m + 1) * (m + 1) <= SLICE * lanes:
        m += 1
    return m


def auto_lanes(goff):
    """The lanes a row's group gets: the smallest power of two that holds the factor's mean m, at most 64."""
    n = len(goff) - 1
    mean = float(goff[-1]) / n if n else 0.0
    lanes = 1
    while lanes < 64 and lanes < mean:
        lanes *= 2
    return lanes


def from_patterns(lower, upper, dtype, seed=0):
    """A non-symmetric matrix from its strict patterns: lower[i] / upper[i] = the columns < i / > i of row i.  The values are awkward
    ones (trisolve_model.awkward) divided by the row's length, each entry's own; the diagonal is 1.5 + u + the larger of the row's and
    the column's absolute sums, so the elimination of every principal square runs without pivoting."""
    rng = np.random.default_rng(seed)
    n = len(lower)
    A = np.zeros((n, n))
    S = np.zeros((n, n), bool)
    for i in range(n):
        cols = np.concatenate([np.asarray(lower[i], np.int64), np.asarray(upper[i], np.int64)])
        A[i, cols] = tm.awkward(rng, len(cols), dtype).astype(np.float64) / max(len(cols), 1)
        S[i, cols] = True
    d = np.arange(n)
    A[d, d] = 1.5 + rng.uniform(size=n) + np.maximum(np.abs(A).sum(axis=1), np.abs(A).sum(axis=0))
    S[d, d] = True
    return tm.from_rows([[(int(c), float(A[i, c])) for c in np.flatnonzero(S[i])] for i in range(n)], dtype)


def ragged(n, period, dtype, seed=0):
    """Row i has i mod period strict-lower entries (as many as there are columns) and up to three strict-upper ones: G_L's rows have
    m = 1 .. period in every residue, G_U's are short."""
    rng = np.random.default_rng(seed)
    return from_patterns([np.sort(rng.choice(i, min(i % period, i), replace=False)) for i in range(n)],
                         [np.sort(rng.choice(np.arange(i + 1, n), min(3, n - 1 - i), replace=False)) for i in range(n)], dtype, seed + 1)


def arrow(n, last, dtype, column, seed=0):
    """The diagonal and a last row (column: a last column) with `last` off-diagonal entries, in the columns (rows) 0 .. last-1."""
    rng = np.random.default_rng(seed)
    v = tm.awkward(rng, last, dtype).astype(np.float64) / last
    d = 1.5 + rng.uniform(size=n)
    if column:
        rows = [[(i, float(d[i]))] + ([(n - 1, float(v[i]))] if i < last else []) for i in range(n - 1)]
        rows.append([(n - 1, float(d[n - 1] + np.abs(v).sum()))])
    else:
        rows = [[(i, float(d[i]))] for i in range(n - 1)]
        rows.append([(c, float(v[c])) for c in range(last)] + [(n - 1, float(d[n - 1] + np.abs(v).sum()))])
    return tm.from_rows(rows, dtype)


# name -> the wrong variants of fsai_ns_model.ORDERS the case can tell from the right one.  "fma" needs an update whose product rounds;
# "column" a square that is not symmetric; "recip" a row of H with m >= 2; "descending" a back-substitution sum of three terms that
# round (m >= 4 and a square that fills: on the five-point grids and the tridiagonal matrix a sum has one non-zero term).  (The arrows'
# squares are diagonal but for one row or column: no update's product is formed from two non-zeros, and the dense last row alone gives
# G_L multipliers that no variant touches and an H of single entries; the dense last column gives H's last row, which "recip" moves, and
# a last pivot that takes B[q][k] for a zero B[k][q].  The grids' few coefficients -- 5, -2, -1, -1.5, -0.5 -- leave most products
# exact: only "column" is promised there.)
_ALL = ("fma", "column", "descending", "recip")
NAMES = {
    "empty": (), "one": (), "diagonal": (),
    "tridiag3000": ("fma", "column", "recip"),
    "dense70": _ALL,
    "ragged": _ALL,
    "random_ns": _ALL,
    "arrow_row128": (),
    "arrow_col128": ("column", "recip"),
    "convdiff12": ("column",),
    "convdiff24": ("column",),
}
REFUSED = {"arrow_row129": ("row", 999), "arrow_col129": ("column", 999)}  # name -> what the refusal names


def matrix(name, dtype):
    """(off, col, val): rows strictly ascending, every diagonal stored."""
    if name == "empty":
        return np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype)
    if name == "one":
        return tm.from_rows([[(0, 2.5)]], dtype)
    if name == "diagonal":
        rng = np.random.default_rng(1)
        return np.arange(301, dtype=np.uint32), np.arange(300, dtype=np.uint32), (1.0 + rng.uniform(size=300)).astype(dtype)
    if name == "tridiag3000":
        return bm.tridiag_ns(3000, 0.5, dtype, seed=2)
    if name == "dense70":  # m = 1 .. 70 in both factors
        return from_patterns([np.arange(i) for i in range(70)], [np.arange(i + 1, 70) for i in range(70)], dtype, seed=3)
    if name == "ragged":  # m = 1 .. 128, twice: every m around every lane width and around every fit(lanes), and the longest row
        return ragged(256, 128, dtype, seed=4)
    if name == "random_ns":  # six columns below and three above the diagonal per row, each triangle's pattern its own
        rng = np.random.default_rng(7)
        n = 200
        return from_patterns([np.sort(rng.choice(i, min(i, 6), replace=False)) for i in range(n)],
                             [np.sort(rng.choice(np.arange(i + 1, n), min(3, n - 1 - i), replace=False)) for i in range(n)], dtype, seed=7)
    if name.startswith("arrow_row"):  # 1000 rows, the last with m = 128 (the most a row may hold) or 129
        return arrow(1000, int(name[9:]) - 1, dtype, False, seed=8)
    if name.startswith("arrow_col"):  # ... the last column: the last row of G_U's H
        return arrow(1000, int(name[9:]) - 1, dtype, True, seed=9)
    if name.startswith("convdiff"):  # the five-point convection-diffusion grids of the solver tests, rows sorted
        return pm.sort_rows(*bm.convdiff2d(int(name[8:]), 1.0, dtype))
    raise KeyError(name)


_FACTORS = {}


def factor(name, dtype):
    """(gl, gu, singular) of the model on the case, computed once and left unchanged."""
    key = name, np.dtype(dtype).name
    if key not in _FACTORS:
        _FACTORS[key] = nm.fsai_ns(*matrix(name, dtype))
    return _FACTORS[key]
