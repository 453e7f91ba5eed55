"""The matrices of the FSAI tests, shared by tests/test_fsai_model.py (CPU: the bounds, and every case moves a bit under each wrong
variant it can tell apart) and tests/test_fsai_gpu.py (the device equals the model bit for bit on the same cases)."""
import numpy as np

import fsai_model as fm
import sgs_model
import trisolve_model as tm

MAX_ROW = fm.MAX_ROW  # kFsaiMaxRow of csrc/fsai.hip: a row with more entries on or below the diagonal is refused
SLICE = 8             # kFsaiSlice: a group of L lanes holds a triangle of at most SLICE * L values in the LDS
LANES = (1, 2, 4, 8, 16, 32, 64)


def fit(lanes):
    """The longest row (m entries on or below the diagonal) whose triangle of m (m + 1) / 2 values fits the slice of `lanes` lanes:
    3, 5, 7, 10, 15, 22, 31.  A longer one is a workgroup's, with the triangle in global scratch."""
    m = 1
    while (m + 1) * (m + 2) // 2 <= SLICE * lanes:
        m += 1
    return m


def auto_lanes(goff):
    """The lanes a row's group gets: the smallest power of two that holds the mean m, at most 64."""
    n = len(goff) - 1
    mean = float(goff[-1]) / n if n else 0.0
    lanes = 1
    while lanes < 64 and lanes < mean:
        lanes *= 2
    return lanes


def spd(lower, dtype, seed=0, upper=None, zeros=0):
    """An SPD matrix from its strict lower pattern: lower[i] = the ascending columns < i of row i.  The values are awkward ones
    (trisolve_model.awkward) divided by the row's length, mirrored into the upper triangle; the diagonal is 1.5 + u + the row's
    absolute sum.  upper: instead of the mirror image, row i's strict upper part has these columns with values of their own (the
    lower triangle alone defines the FSAI).  zeros: that many stored off-diagonal pairs are set to 0."""
    rng = np.random.default_rng(seed)
    n = len(lower)
    A = np.zeros((n, n))
    S = np.zeros((n, n), bool)
    for i, cols in enumerate(lower):
        cols = np.asarray(cols, np.int64)
        v = tm.awkward(rng, len(cols), dtype).astype(np.float64) / max(len(cols), 1)
        A[i, cols] = v
        S[i, cols] = True
    if zeros:
        r, c = np.nonzero(S)
        pick = rng.choice(len(r), zeros, replace=False)
        A[r[pick], c[pick]] = 0.0
    A = A + A.T
    S = S | S.T
    A[np.arange(n), np.arange(n)] = 1.5 + rng.uniform(size=n) + np.abs(A).sum(axis=1)
    S[np.arange(n), np.arange(n)] = True
    if upper is not None:
        for i, cols in enumerate(upper):
            S[i, i + 1:] = False
            cols = np.asarray(cols, np.int64)
            S[i, cols] = True
            A[i, cols] = tm.awkward(rng, len(cols), dtype)
    return tm.from_rows([[(int(c), float(A[i, c])) for c in np.flatnonzero(S[i])] for i in range(n)], dtype)


def ragged(n, period, dtype, seed=0):
    """Row i has i mod period strict-lower entries (as many as there are columns), so m = 1 .. period in every residue."""
    rng = np.random.default_rng(seed)
    return spd([np.sort(rng.choice(i, min(i % period, i), replace=False)) for i in range(n)], dtype, seed + 1)


def dense(n, dtype, seed=0):
    return spd([np.arange(i) for i in range(n)], dtype, seed)


def arrow(n, last, dtype, seed=0):
    """The diagonal and a last row (and column) with `last` strict-lower entries: the columns 0 .. last-1."""
    rng = np.random.default_rng(seed)
    v = tm.awkward(rng, last, dtype).astype(np.float64) / last
    d = 1.5 + rng.uniform(size=n)
    rows = [[(i, float(d[i] + (abs(v[i]) if i < last else 0.0)))] + ([(n - 1, float(v[i]))] if i < last else []) for i in range(n - 1)]
    rows.append([(c, float(v[c])) for c in range(last)] + [(n - 1, float(d[n - 1] + np.abs(v).sum()))])
    return tm.from_rows(rows, dtype)


def lap3d(nx, ny, nz, dtype, seed=0, spread=1.0):
    """sgs_model.lap2d's operator on an nx x ny x nz grid: a 7-point stencil with edge weights 10^U(-spread/2, spread/2)."""
    rng = np.random.default_rng(seed)
    n = nx * ny * nz
    idx = np.arange(n).reshape(nx, ny, nz)
    ea = np.concatenate([idx[:-1].ravel(), idx[:, :-1].ravel(), idx[:, :, :-1].ravel()])
    eb = np.concatenate([idx[1:].ravel(), idx[:, 1:].ravel(), idx[:, :, 1:].ravel()])
    w = 10.0 ** rng.uniform(-spread / 2, spread / 2, len(ea))
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


# name -> the wrong variants of fsai_model.ORDERS the case can tell from the right one.  "fma" needs an update whose product
# rounds; "recip" and "div_sqrt" a row with m >= 2; "descending" a back-substitution sum of three terms that round (m >= 4 and a
# triangle that fills: on the five-point grids a sum has one non-zero term); "upper" an upper triangle that is not the lower's mirror
# image.  (table0 has unit weights: every product is exact and a multiplier is -1 / pivot either way, so only the scaling shows.  The
# arrow's last pivot takes 127 products, each far below its last place.  "two" has too few roundings to promise a difference.)
_ALL = ("fma", "descending", "recip", "div_sqrt")
NAMES = {
    "empty": (), "one": (), "two": (), "diagonal": (),
    "chain3000": ("fma", "recip", "div_sqrt"),
    "dense70": _ALL, "dense128": _ALL, "ragged": _ALL,
    "lap3d12": ("fma", "recip", "div_sqrt"),
    "stored_zeros": _ALL,
    "nonsymmetric": _ALL + ("upper",),
    "arrow128": ("recip", "div_sqrt"),
}
for _k in range(len(sgs_model.TABLE)):
    NAMES["table%d" % _k] = NAMES["table%d-rb" % _k] = ("fma", "recip", "div_sqrt") if sgs_model.TABLE[_k][2] else ("div_sqrt",)
REFUSED = {"dense129": 128, "arrow5001": 5000}  # name -> the row the refusal names


def matrix(name, dtype):
    """(off, col, val): rows strictly ascending, every diagonal stored."""
    if name == "empty":
        return np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype)
    if name == "one":
        return tm.from_rows([[(0, 2.5)]], dtype)
    if name == "two":
        return tm.from_rows([[(0, 2.5), (1, -0.7)], [(0, -0.7), (1, 3.1)]], dtype)
    if name == "diagonal":
        rng = np.random.default_rng(1)
        return np.arange(301, dtype=np.uint32), np.arange(300, dtype=np.uint32), (1.0 + rng.uniform(size=300)).astype(dtype)
    if name == "chain3000":
        return spd([[i - 1] if i else [] for i in range(3000)], dtype, seed=2)
    if name.startswith("dense"):  # m = 1 .. n
        return dense(int(name[5:]), dtype, seed=3)
    if name == "ragged":  # m = 1 .. 70, four times: every m around every lane width and around every fit(lanes)
        return ragged(280, 70, dtype, seed=4)
    if name.startswith("table"):
        off, col, val, _, _ = sgs_model.table_case(int(name[5]), "red_black" if name.endswith("-rb") else "natural")
        return off, col, val.astype(dtype)
    if name == "lap3d12":
        return lap3d(12, 12, 12, dtype, seed=5)
    if name == "stored_zeros":  # a symmetric pattern of which 40 stored pairs hold 0
        rng = np.random.default_rng(6)
        return spd([np.sort(rng.choice(i, min(i, 5), replace=False)) for i in range(150)], dtype, seed=6, zeros=40)
    if name == "nonsymmetric":  # the strict upper part: three columns of its own per row, other values
        rng = np.random.default_rng(7)
        n = 200
        return spd([np.sort(rng.choice(i, min(i, 6), replace=False)) for i in range(n)], dtype, seed=7,
                   upper=[np.sort(rng.choice(np.arange(i + 1, n), min(3, n - 1 - i), replace=False)) for i in range(n)])
    if name == "arrow128":  # 200 rows, the last with m = 128: the most a row may hold
        return arrow(200, 127, dtype, seed=8)
    if name == "arrow5001":  # ... with m = 5001
        return arrow(5001, 5000, dtype, seed=9)
    raise KeyError(name)


_FACTORS = {}


def factor(name, dtype):
    """(goff, gcol, gval, not_spd) of the model on the case, computed once and left unchanged."""
    key = name, np.dtype(dtype).name
    if key not in _FACTORS:
        _FACTORS[key] = fm.fsai(*matrix(name, dtype))
    return _FACTORS[key]
