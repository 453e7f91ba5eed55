"""Special values and gradual underflow in y = A x: the inputs the GPU tests feed the kernels (seeded, so that the CPU tests can
hold the very same data against the oracle), a CLASS MODEL of the result that does not depend on the order of summation, and
the derived bound for sums of subnormal products.

The class of a row (tests/util.py::value_class: 0 finite, 1 +Inf, 2 -Inf, 3 NaN), with p = val * x[col] in the matrix's type:
NaN if any p is NaN or +Inf and -Inf both occur; else +Inf if a +Inf occurs; else -Inf if a -Inf occurs; else finite.  As long
as no sum of FINITE products can overflow this is what every order of additions gives.  The inputs here guarantee that: every
finite value and every finite x_j is at most 1 in magnitude and rows are shorter than 2^20 entries."""
import numpy as np

import oracle
from util import EPS, exact_row_sums, random_crs, value_class

SEED_MATRIX = 0x5EED0001   # (sparsemat_amd.synth.SEED_MATRIX: the generated matrices of the benchmark)
SLICE = 16384              # (tiled_model.SLICE: columns per K2t slice)
X_TAIL = 37                # x_single is this much longer than n_cols, the tail being NaN
SPECIALS = (np.inf, -np.inf, np.nan)


def row_classes(off, col, val, x):
    """The class model: one multiply per entry in the matrix's type, then counting -- no sum is formed."""
    dt = np.dtype(val.dtype)
    n_rows = len(off) - 1
    out = np.zeros(n_rows, np.int8)
    if not len(val):
        return out
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = (val * np.asarray(x, dt)[col]).astype(dt)
    assert (np.abs(p[np.isfinite(p)]) <= 1).all() and np.diff(off.astype(np.int64)).max() < (1 << 20)   # (no finite sum overflows)
    starts = off[:-1].astype(np.int64)
    nonempty = np.diff(off.astype(np.int64)) > 0
    cnt = {}
    for name, hit in (("nan", np.isnan(p)), ("pinf", np.isposinf(p)), ("ninf", np.isneginf(p))):
        c = np.zeros(n_rows, np.int64)
        c[nonempty] = np.add.reduceat(hit.astype(np.int64), starts[nonempty])
        cnt[name] = c
    out[cnt["ninf"] > 0] = 2
    out[cnt["pinf"] > 0] = 1
    out[(cnt["nan"] > 0) | ((cnt["pinf"] > 0) & (cnt["ninf"] > 0))] = 3
    return out


def dot_class(lhs, y):
    """The class of lhs . y by the same counting (|lhs_i| <= 1, |y_i| at most a row's length: no finite sum overflows)."""
    with np.errstate(invalid="ignore"):
        p = lhs * y
    nan, pinf, ninf = np.isnan(p).any(), np.isposinf(p).any(), np.isneginf(p).any()
    return 3 if nan or (pinf and ninf) else 1 if pinf else 2 if ninf else 0


def finite_share(off, cls):
    """Share of the NON-EMPTY rows whose class is finite."""
    nonempty = np.diff(off.astype(np.int64)) > 0
    return float((cls[nonempty] == 0).mean())


# ---- the unusual data (structure is never touched: every column index stays valid) ---------------------------------------------
def x_sparse(seed, n_cols, dtype, share):
    """Uniform in [-1, 1] with a random `share` of the columns +Inf, -Inf or NaN."""
    rng = np.random.default_rng([seed, 1])
    x = rng.uniform(-1, 1, n_cols).astype(dtype)
    hit = rng.random(n_cols) < share
    x[hit] = np.array(SPECIALS, dtype)[rng.integers(0, 3, int(hit.sum()))]
    return x


def x_single(seed, off, col, n_cols, dtype, inf_col=None):
    """Finite but for: ONE referenced column +Inf (by default one that no row of more than 1000 entries references, where there is
    such a column), every column no row references NaN, and a NaN tail of X_TAIL elements beyond n_cols.  Returns (x, the column)."""
    rng = np.random.default_rng([seed, 2])
    x = np.concatenate([rng.uniform(-1, 1, n_cols), np.full(X_TAIL, np.nan)]).astype(dtype)
    used = np.zeros(n_cols, bool)
    used[col] = True
    x[:n_cols][~used] = np.nan
    if inf_col is None:
        lens = np.diff(off.astype(np.int64))
        in_long = np.zeros(n_cols, bool)
        in_long[col[np.repeat(lens > 1000, lens)]] = True
        cand = np.nonzero(used & ~in_long)[0]
        if not len(cand):
            cand = np.nonzero(used)[0]
        inf_col = int(cand[rng.integers(0, len(cand))])
    assert used[inf_col]
    x[inf_col] = np.inf
    return x, inf_col


def val_special(seed, val):
    """0.5 % of the stored values from {+Inf, -Inf, NaN}, 1 % of them +0.0 or -0.0 (at least one of each of the five)."""
    rng = np.random.default_rng([seed, 3])
    out = val.copy()
    n = len(val)
    where = rng.permutation(n)
    n_sp, n_z = max(3, n // 200), max(2, n // 100)
    sp = np.array(SPECIALS, val.dtype)[rng.integers(0, 3, n_sp)]
    sp[:3] = SPECIALS
    z = np.array([0.0, -0.0], val.dtype)[rng.integers(0, 2, n_z)]
    z[:2] = (0.0, -0.0)
    out[where[:n_sp]] = sp
    out[where[n_sp:n_sp + n_z]] = z
    return out


def x_finite(seed, n_cols, dtype):
    return np.random.default_rng([seed, 4]).uniform(-1, 1, n_cols).astype(dtype)


def inputs(name, dtype):
    """(tag, values, x) for every special-value run of matrix `name`: x_sparse, x_single, val_special with a finite x and with
    x_sparse (stored zeros meet Inf there: 0 * Inf = NaN)."""
    n_rows, n_cols, off, col, val, share = matrix(name, dtype)
    seed = sum(name.encode()) * 2 + (np.dtype(dtype) == np.dtype(np.float64))
    xs = x_sparse(seed, n_cols, dtype, share)
    vs = val_special(seed, val)
    return [("x_sparse", val, xs), ("x_single", val, x_single(seed, off, col, n_cols, dtype)[0]),
            ("val_special", vs, x_finite(seed, n_cols, dtype)), ("val_special+x_sparse", vs, xs)]


# ---- the matrices: each the smallest shape an existing test uses to force one kernel form -------------------------------------
def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    return off


def _band(rng, n, lens, half, dtype):
    off = _offsets(lens)
    centers = np.repeat(np.arange(n), lens)
    col = np.clip(centers + rng.integers(-half, half, len(centers)), 0, n - 1).astype(np.uint32)
    return n, n, off, col, rng.uniform(-1, 1, len(col)).astype(dtype)


def _laplace(g, dtype, scale=1.0):
    """A 7-point stencil with values of magnitude <= 1 (the Laplacian's 6 / -1 times 1/8: exact, and still two distinct values)."""
    off, col, val = oracle.laplace3d(*g, dtype)
    n = g[0] * g[1] * g[2]
    return n, n, off, col, (val * dtype(0.125 * scale)).astype(dtype)


WIDE_RING_ROWS = 30_000          # rows of the +-10000 band at which the plan takes the 32768-column ring (f32; at 24 000 it does not)
BANDED_RING_GRID = (130, 130, 5)  # planes 16900 columns apart: beyond half of either ring -> four bands
PAR_ROWS, PAR_K, PAR_BAND = 30_011, 16, 700


def matrix(name, dtype):
    """(n_rows, n_cols, off, col, val, share of x_sparse's columns that are non-finite)."""
    rng = np.random.default_rng(sum(name.encode()))
    if name == "ragged3001":         # test_random_matrices_all_variants' shape, ragged and skewed at once
        n_rows, n_cols = 3001, 2777
        lens = rng.integers(0, 70, n_rows)
        lens[1500], lens[2203] = 2049 + 551, 5000
        lens[3] += lens.sum() % 4 == 0   # (borrowed device arrays then end inside a 16-byte chunk)
        return (n_rows, n_cols) + random_crs(rng, n_rows, n_cols, lens, dtype, dup=True) + (0.015,)
    if name == "banded3000x7":       # K1r, one window
        return (3000, 3000) + oracle.gen_fixed(SEED_MATRIX, oracle.PATTERN_BANDED, 3000, 7, dtype) + (0.05,)
    if name == "wide_band":          # K1r, the 32768-column ring (f32)
        return _band(rng, WIDE_RING_ROWS, rng.integers(20, 45, WIDE_RING_ROWS), 10_000, dtype) + (0.01,)
    if name == "stencil_planes":     # K1r, four bands
        return _laplace(BANDED_RING_GRID, dtype) + (0.05,)
    if name == "stencil48":          # K1s coded / XS / XD / XD-V: 2048-entry stage, most rows of odd length
        return _laplace((48, 20, 9), dtype) + (0.05,)
    if name == "stencil1000":        # ... the 4096-entry stage
        return _laplace((1000, 30, 3), dtype) + (0.05,)
    if name == "xd_long_rows":       # rows of 5 entries with one of 23 / 40 now and then: K1s XD's loop after the eight masked adds
        n = 20_000
        lens = np.full(n, 5)
        lens[::64], lens[37::640] = 23, 40
        return _band(rng, n, lens, 250, dtype) + (0.05,)
    if name == "colblock6007":       # K2c / K2f: 20 column blocks at shift 8
        n_rows, n_cols = 6007, 5001
        return (n_rows, n_cols) + random_crs(rng, n_rows, n_cols, rng.integers(0, 70, n_rows), dtype, dup=True) + (0.015,)
    if name == "colsplit9001":       # K2s: a minority of long rows
        n_rows, n_cols = 9001, 7003
        lens = rng.integers(0, 12, n_rows)
        heavy = rng.random(n_rows) < 0.04
        lens[heavy] = rng.integers(64, 700, heavy.sum())
        lens[11], lens[12] = 63, 64
        return (n_rows, n_cols) + random_crs(rng, n_rows, n_cols, lens, dtype, dup=True) + (0.05,)
    if name == "tiled_skewed":       # K2t: 5 slices, the last short; one row cut by chunk boundaries in every slice
        n_rows, n_cols = 6007, 5 * SLICE - 331
        lens = rng.integers(0, 6, n_rows)
        lens[17] = 9000
        lens[4000:4100] = 300
        return (n_rows, n_cols) + random_crs(rng, n_rows, n_cols, lens, dtype, dup=True) + (0.12,)
    if name == "tiled_rounds":       # K2t: every column in the first of four slices -> tiles of several rounds
        n_rows = 9000
        return (n_rows, 4 * SLICE) + random_crs(rng, n_rows, SLICE - 7, rng.integers(1, 4, n_rows), dtype) + (0.15,)
    if name == "tiled_64chunks":     # K2t: one slice of 16 holds every entry, 1013 chunks = 64 per wavefront
        n_rows, chunks = 8000, 1013
        total = 240 * chunks - 57
        lens = np.full(n_rows, total // n_rows)
        lens[: total - lens.sum()] += 1
        off, col, val = random_crs(rng, n_rows, SLICE - 3, lens, dtype)
        return (n_rows, 16 * SLICE, off, (col + 3 * SLICE).astype(np.uint32), val, 0.01)
    if name == "par_banded":         # the partitioned product: 16 entries per row within +-700
        n = PAR_ROWS
        off = np.arange(n + 1, dtype=np.uint32) * PAR_K
        base = np.arange(n, dtype=np.int64)[:, None] + rng.integers(-PAR_BAND, PAR_BAND + 1, (n, PAR_K))
        return (n, n, off, np.clip(base, 0, n - 1).astype(np.uint32).reshape(-1), rng.uniform(-1, 1, n * PAR_K).astype(dtype), 0.03)
    raise ValueError(name)


# columns of x no row references (x_single makes them NaN): whole K2t slices, the gaps of a band
UNREFERENCED_AT_LEAST = {"tiled_skewed": 50_000, "tiled_rounds": 3 * SLICE, "tiled_64chunks": 15 * SLICE, "xd_long_rows": 100, "banded3000x7": 10}

MATRICES = ("ragged3001", "banded3000x7", "wide_band", "stencil_planes", "stencil48", "stencil1000", "xd_long_rows", "colblock6007",
            "colsplit9001", "tiled_skewed", "tiled_rounds", "tiled_64chunks", "par_banded")


def merge_long_row(dtype, where):
    """test_edge_shapes' 6 x 10000 matrix, the long row at 9001 entries: all data finite but ONE value of that row, +Inf -- its
    first entry (the row's first merge tile: the Inf travels through the carry fix-up) or its last."""
    rng = np.random.default_rng(3)
    off, col, val = random_crs(rng, 6, 10000, np.array([0, 0, 9001, 0, 1, 0]), dtype)
    x = rng.uniform(-1, 1, 10000).astype(dtype)
    x[x == 0] = 0.5
    val[int(off[2]) if where == "first" else int(off[3]) - 1] = np.inf
    return off, col, val, x


# ---- gradual underflow -----------------------------------------------------------------------------------------------------------
UNDERFLOW_MATRICES = ("ragged3001", "stencil48", "banded3000x7", "tiled_skewed", "colblock6007", "colsplit9001")
Q = {np.dtype(np.float32): 2.0 ** -149, np.dtype(np.float64): 2.0 ** -1074}   # the spacing of the subnormal numbers


def underflow_inputs(name, dtype, positive):
    """Values times 2^-70 and x times 2^-65 (f64: 2^-520, 2^-515): every product is subnormal and the row sums straddle the smallest
    normal number.  `positive`: all values and all of x positive, so that no exact row sum is small against sum|a x|."""
    n_rows, n_cols, off, col, val, _ = matrix(name, dtype)
    x = x_finite(sum(name.encode()) + 77, n_cols, dtype)
    if positive:
        val, x = np.abs(val), np.abs(x)
    e_val, e_x = (-70, -65) if np.dtype(dtype) == np.dtype(np.float32) else (-520, -515)
    val, x = np.ldexp(val, e_val).astype(dtype), np.ldexp(x, e_x).astype(dtype)
    with np.errstate(under="ignore"):
        p = val * x[col]
    assert (np.abs(p) < np.finfo(dtype).tiny).all() and (p != 0).mean() > 0.9   # subnormal, and not simply zero
    return n_rows, n_cols, off, col, val, x


def underflow_bound(off, col, val, x):
    """(exact row sums, bound) with |y - exact| <= L q + 2 L eps sum|a x| per row of length L: each product errs by at most q / 2
    (subnormal result) or eps |p|, each add is exact while the sum is subnormal and errs by at most eps sum|a x| otherwise.
    Derived, not measured; both in the wide type of exact_row_sums (f64 for f32 data, long double for f64 data)."""
    dt = np.dtype(val.dtype)
    exact = exact_row_sums(off, col, val, x)
    sum_abs = exact_row_sums(off, col, np.abs(val), np.abs(x))
    lens = np.diff(off.astype(np.int64)).astype(exact.dtype)
    wide = exact.dtype.type
    return exact, lens * wide(Q[dt]) + 2 * lens * wide(EPS[dt]) * sum_abs


def underflow_ratio(y, exact, bound):
    """max over the non-empty rows of |y - exact| / bound (NaN if y holds one); empty rows must be exactly +0."""
    nonempty = bound > 0
    assert not y[~nonempty].any() and not np.signbit(y[~nonempty]).any()
    with np.errstate(invalid="ignore"):
        r = np.abs(y[nonempty].astype(exact.dtype) - exact[nonempty]) / bound[nonempty]
    return float(r.max()) if not np.isnan(r).any() else float("nan")
