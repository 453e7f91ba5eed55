"""The matrices and kernel forms that the bit-for-bit tests share (tests/test_solver_kernels_gpu.py, tests/test_spmv_order_gpu.py and,
on the CPU, tests/test_spmv_order_model.py): the builders, CONFIGS -- per product kernel form the matrix, the variant, the handle's
knobs and what its getters must report -- and the cases of the summation-order tests.  Nothing here touches the device."""
import contextlib
import functools
import os

import numpy as np

import oracle

F32, F64 = np.float32, np.float64


def same(a, b):
    """bit equality (any NaN equals any NaN: its sign and payload are not arithmetic)"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- the matrices ------------------------------------------------------------------------------------------------------------
def crs_from_pattern(n, rows, cols, zero, dtype, shuffle_seed=None):
    """(off, col, val) from the distinct positions (rows[k], cols[k]) -- every diagonal position among them.  zero[k]: a stored
    0.0.  Off-diagonal values -w(min(i, j), max(i, j)), w in (0, 1): symmetric; a_ii = 1 + sum_j |a_ij| (summed in f64 from the
    rounded off-diagonals).  Rows ascending, or in random order (shuffle_seed)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    minor = cols if shuffle_seed is None else np.random.default_rng(shuffle_seed).permutation(len(rows))
    order = np.lexsort((minor, rows))
    rows, cols, zero = rows[order], cols[order], np.asarray(zero, bool)[order]
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    w = ((lo * 2654435761 + hi * 40503) % 1000003 + 1) / 1000004.0
    val = np.where(zero | (rows == cols), 0.0, -w).astype(dtype)
    diag = 1.0 + np.bincount(rows, weights=np.abs(val.astype(np.float64)), minlength=n)
    on_diag = rows == cols
    assert on_diag.sum() == n and not zero[on_diag].any()
    val[on_diag] = diag.astype(dtype)
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(np.bincount(rows, minlength=n), out=off[1:])
    return off, cols.astype(np.uint32), val


@functools.lru_cache(maxsize=None)
def band_pattern(n, w, length):
    rng = np.random.default_rng(n + w)
    d = np.concatenate([[1], np.sort(rng.choice(np.arange(2, w), 13, replace=False)), [w]])
    offs = np.concatenate([-d[::-1], [0], d])
    taken = set(offs.tolist())
    free = [t for k in range(2, 60) for t in (k, -k) if t not in taken]  # where the stored zeros go: next to the diagonal
    i = np.arange(n)
    cand = i[:, None] + offs[None, :]
    valid = (cand >= 0) & (cand < n)
    rows = [np.broadcast_to(i[:, None], cand.shape)[valid]]
    cols = [cand[valid]]
    zero = [np.zeros(int(valid.sum()), bool)]
    need = length - valid.sum(axis=1)
    inner = np.flatnonzero((need == 1) & (i + free[0] < n))  # (length 32: one zero per row, to the right where there is room)
    rows.append(inner)
    cols.append(inner + free[0])
    zero.append(np.ones(len(inner), bool))
    need[inner] = 0
    pr, pc = [], []
    for r in np.flatnonzero(need):
        got = [r + t for t in free if 0 <= r + t < n][:need[r]]
        assert len(got) == need[r]
        pr += [r] * len(got)
        pc += got
    rows.append(np.array(pr, np.int64))
    cols.append(np.array(pc, np.int64))
    zero.append(np.ones(len(pr), bool))
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(zero)


def band(n, w, length, dtype):
    off, col, val = crs_from_pattern(n, *band_pattern(n, w, length), dtype)
    assert (np.diff(off.astype(np.int64)) == length).all() and int(np.abs(col.astype(np.int64) - np.repeat(np.arange(n), length)).max()) == w
    return off, col, val


def symmetric_positions(n, r, c):
    """the distinct positions (i, j), (j, i) of the pairs and the whole diagonal"""
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    key = np.unique(lo[lo != hi] * n + hi[lo != hi])
    lo, hi = key // n, key % n
    d = np.arange(n)
    return np.concatenate([lo, hi, d]), np.concatenate([hi, lo, d])


@functools.lru_cache(maxsize=None)
def scattered_pattern(n, hubs):
    rng = np.random.default_rng(n)
    r, c = [np.repeat(np.arange(n), 4)], [rng.integers(0, n, 4 * n)]
    if hubs:
        for h in range(0, n, 997):
            r.append(np.full(3000, h))
            c.append(rng.choice(n, 3000, replace=False))
    return symmetric_positions(n, np.concatenate(r), np.concatenate(c))


def scattered(n, dtype, hubs=True):
    rows, cols = scattered_pattern(n, hubs)
    return crs_from_pattern(n, rows, cols, np.zeros(len(rows), bool), dtype, shuffle_seed=1)


@functools.lru_cache(maxsize=None)
def arrowhead_pattern(n):
    rng = np.random.default_rng(n)
    r, c = [np.repeat(np.arange(n), 2)], [rng.integers(0, n, 2 * n)]
    for h in range(n // 80, n, n // 40):
        r.append(np.full(2000, h))
        c.append(rng.choice(n, 2000, replace=False))
    return symmetric_positions(n, np.concatenate(r), np.concatenate(c))


def arrowhead(n, dtype):
    rows, cols = arrowhead_pattern(n)
    return crs_from_pattern(n, rows, cols, np.zeros(len(rows), bool), dtype, shuffle_seed=2)


def stencil7(g, dtype):
    off, col, _ = oracle.laplace3d(*g, dtype)
    n = len(off) - 1
    rows = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    got = crs_from_pattern(n, rows, col, np.zeros(len(col), bool), dtype)
    assert np.array_equal(got[0], off) and np.array_equal(got[1], col)  # (the oracle's rows are ascending already)
    return got


# ---- the configurations ------------------------------------------------------------------------------------------------------
class Config:
    """build(dtype) -> (off, col, val); variant; knobs(m): the handle's setters; env: the environment knobs, set through the whole
    case; check(m): what the getters must report (asserted after prepare and again after the solves); fused: CG and PCG take p.Ap
    from the K1s epilogue; same_as: an "auto" case's explicitly named variant, whose solves must give the same bytes."""

    def __init__(self, build, variant, check, knobs=None, env=None, dtypes=(F32, F64), fused=False, same_as=None, stop=F32):
        self.build, self.variant, self.check, self.knobs, self.env = build, variant, check, knobs or (lambda m: None), env or {}
        self.dtypes, self.fused, self.same_as, self.stop = dtypes, fused, same_as, stop


NO_RING_ENV = dict(SMH_RING_COL16=None, SMH_RING_COL12=None)


def k1(lanes):
    def knobs(m):
        m.set_ring(0)
        m.set_vector_lanes(lanes)

    def check(m):
        assert m.resolved_variant() == ("vector", lanes) and not m.ring_plan()[2] and m.ring_column_form() == "u32"
    return knobs, check


def ring(form, entries=16384, bands=1, force=True):
    def knobs(m):
        if force:
            m.set_ring(1)

    def check(m):
        assert m.ring_plan()[2] and m.ring_plan()[1] >= 0.5, m.ring_plan()[:3]   # active, and most rows served from the ring
        assert (m.ring_column_form(), m.ring_entries(), m.ring_bands()) == (form, entries, bands)
    return knobs, check


def blocks13(m):
    m.set_colblock_shift(13)


def check_merge(m):
    assert len(m.merge_table()[0]) - 1 > 1


def check_colblock(m):
    assert m.colblock(arrays=False)["n_blocks"] == 5


def check_colfused(m):
    cf = m.colfused(arrays=False)
    assert cf["fits"] and cf["n_blocks"] == 5, cf  # (fits: K2f itself runs, not the fall-through to the per-block launches)


def check_colsplit(m):
    sp = m.colsplit()
    assert sp["split"] and sp["n_long"] == 40 and sp["long"][0] == 40 and sp["short"][0] == m.n_rows(), (sp["split"], sp["n_long"])


def check_tiled(m):
    assert m.tiled_layout()["n_slices"] == 3


def stream_form(xs, direct, n_dict):
    def check(m):
        lay = m.stream_layout()
        assert lay["coded"] and (lay["xs_chunks"] in (2, 4)) == xs and lay["xs_chunks"] in (0, 2, 4), lay
        assert m.stream_direct() == direct and len(m.stream_value_dict()) == n_dict
    return check


def stream_knobs(xs, direct=-1, vdict=-1):
    def knobs(m):
        m.set_stream_xs(xs)
        m.set_stream_direct(direct)
        m.set_stream_value_dict(vdict)
    return knobs


def resolves_to(name, then=lambda m: None):
    def check(m):
        assert m.resolved_variant()[0] == name
        then(m)
    return check


def laplace24(dtype):
    return oracle.laplace3d(24, 24, 24, dtype)


B31 = functools.partial(band, 20_000, 4000, 31)
B32 = functools.partial(band, 20_000, 4000, 32)
S = functools.partial(scattered, 40_000)
A = functools.partial(arrowhead, 8000)

CONFIGS = {
    # 1. K1 without the ring
    "k1-lanes1": Config(B31, "vector", k1(1)[1], k1(1)[0], NO_RING_ENV),
    "k1-lanes8": Config(B32, "vector", k1(8)[1], k1(8)[0], NO_RING_ENV, stop=F64),
    "k1-lanes32": Config(B31, "vector", k1(32)[1], k1(32)[0], NO_RING_ENV),
    # 2. K1r on one sliding window of 16384 columns, by column form (col12 forced on rows of 31: every chunk straddles two rows, so
    #    every chunk leaves the code through the escape table)
    "k1r-u32": Config(B32, "vector", ring("u32")[1], ring("u32")[0], dict(SMH_RING_COL16="0", SMH_RING_COL12=None), stop=F64),
    "k1r-col16": Config(B32, "vector", ring("col16")[1], ring("col16")[0], dict(SMH_RING_COL16=None, SMH_RING_COL12="0")),
    "k1r-col12-forced": Config(B31, "vector", ring("col12")[1], ring("col12")[0], dict(SMH_RING_COL16=None, SMH_RING_COL12="1"), (F32,)),
    # 3. ... and the compact form taken by itself (neither variable set, the ring not forced)
    "k1r-col12-auto": Config(B32, "vector", ring("col12")[1], ring("col12", force=False)[0], NO_RING_ENV, (F32,)),
    # 4. the wide ring: offsets up to 10 000, 20 064 columns under a 64-row tile.  48 000 rows: near the matrix' edges the band is
    #    cut off, 16 384 columns still hold about 16 000 rows' tiles, and the plan goes wide only where they are under half of the
    #    rows (at 30 000 rows the 16 384-column ring serves 53 % and stays)
    "k1r-wide": Config(functools.partial(band, 48_000, 10_000, 32), "vector", ring("col16", 32768)[1], ring("col16", 32768)[0], NO_RING_ENV, (F32,)),
    # 5. the banded ring: planes of 130 x 130 = 16 900 rows, so a tile's three column intervals lie further apart than any single
    #    window reaches (33 864 columns; the wide ring holds 32 768), and six planes, so that the rows of the two boundary planes,
    #    which the wide ring does hold, are a third of all
    "k1r-banded": Config(functools.partial(stencil7, (130, 130, 6)), "vector", ring("col16", 16384, 4)[1], ring("col16", 16384, 4)[0], NO_RING_ENV,
                         stop=F64),
    "merge": Config(S, "merge", check_merge),                                                   # 6.
    "colblock": Config(S, "colblock", check_colblock, blocks13, stop=F64),                     # 7.
    "colfused": Config(functools.partial(scattered, 40_000, hubs=False), "colfused", check_colfused, blocks13),  # 8.
    "colsplit": Config(A, "colsplit", check_colsplit, stop=F64),                                # 9.
    "tiled": Config(S, "tiled", check_tiled),                                                   # 10.
    # 11. the K1s forms (x is far below the size at which the stage is automatic: forced)
    "k1s-xdv": Config(laplace24, "stream", stream_form(True, True, 2), stream_knobs(1), fused=True),
    "k1s-xd": Config(laplace24, "stream", stream_form(True, True, 0), stream_knobs(1, -1, 0), fused=True, stop=F64),
    "k1s-xs": Config(laplace24, "stream", stream_form(True, False, 0), stream_knobs(1, 0), fused=True),
    "k1s-plain": Config(laplace24, "stream", stream_form(False, False, 0), stream_knobs(0), fused=True, stop=F64),
    # 12. what AUTO takes by itself
    "auto-band": Config(B32, "auto", resolves_to("vector", ring("col12")[1]), env=NO_RING_ENV, dtypes=(F32,), same_as="vector"),
    "auto-arrowhead": Config(A, "auto", resolves_to("merge", check_merge), same_as="merge"),
    "auto-laplace": Config(laplace24, "auto", resolves_to("stream", stream_form(False, False, 0)), fused=True, same_as="stream", stop=F64),
}


# ---- the cases of the summation-order tests (test_spmv_order_model.py on the CPU, test_spmv_order_gpu.py on the device) --------
LANES = (1, 2, 4, 8, 16, 32, 64)
RAGGED_ROWS = 4101          # no multiple of 8 * (256 / lanes) for any lanes (the smallest of them is 32)
RAGGED_LAST_ROW = 37        # entries of the last row before the ones that set nnz mod 4
# the vector-family entries of CONFIGS and the lanes per row their handles resolve to (the device test asserts them against
# resolved_variant(): 8 lanes for a mean row of 31 or 32 entries, 4 for the stencil's 7)
VECTOR_CONFIG_LANES = {"k1-lanes1": 1, "k1-lanes8": 8, "k1-lanes32": 32, "k1r-u32": 8, "k1r-col16": 8, "k1r-col12-forced": 8,
                       "k1r-col12-auto": 8, "k1r-wide": 8, "k1r-banded": 4, "auto-band": 8}


def vector_x(n_cols, dtype, seed=7):
    return np.random.default_rng(seed).uniform(-1, 1, n_cols).astype(dtype)


@functools.lru_cache(maxsize=None)
def ragged_pattern(nnz_mod):
    """(off, col): RAGGED_ROWS rows whose lengths cycle through 0 ... 9, through 4L - 1, 4L, 4L + 1 and 8L + 1 for every L in LANES, and
    through 515; rows 1000 ... 1320 empty; the last row RAGGED_LAST_ROW entries and up to three more, so that nnz mod 4 == nnz_mod.
    The cycle's 3107 entries are an odd number: every row length meets every start s mod 4.  Columns within 1500 of the diagonal."""
    n = RAGGED_ROWS
    cycle = list(range(10)) + [v for L in LANES for v in (4 * L - 1, 4 * L, 4 * L + 1, 8 * L + 1)] + [515]
    lens = np.array([cycle[i % len(cycle)] for i in range(n)], np.int64)
    lens[1000:1321] = 0
    lens[-1] = RAGGED_LAST_ROW
    lens[-1] += (nnz_mod - int(lens.sum())) % 4
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    assert int(off[-1]) % 4 == nnz_mod
    rng = np.random.default_rng(4101)
    rows = np.repeat(np.arange(n), lens)
    col = np.clip(rows + rng.integers(-1500, 1501, len(rows)), 0, n - 1).astype(np.uint32)
    return off, col


def ragged(dtype, nnz_mod=0):
    """(n_cols, off, col, val) of the ragged matrix; some stored +0.0 and -0.0 among the values"""
    off, col = ragged_pattern(nnz_mod)
    val = np.random.default_rng(11).uniform(-1, 1, len(col)).astype(dtype)
    val[::97] = 0.0
    val[5::193] = -0.0
    return RAGGED_ROWS, off, col, val


@functools.lru_cache(maxsize=None)
def mixed_phases_pattern():
    rng = np.random.default_rng(99)
    n_rows, n_cols = 40_000, 300_000
    lens = rng.integers(0, 40, size=n_rows)
    lens[5000:5600] = 0
    off = np.zeros(n_rows + 1, dtype=np.uint32)
    np.cumsum(lens, out=off[1:])
    col = np.empty(int(off[-1]), dtype=np.uint32)
    centers = np.linspace(0, n_cols - 1, n_rows)
    centers[20_000:30_000] = np.linspace(100_000, 0, 10_000)  # runs backwards
    for i in range(n_rows):
        a, b = off[i], off[i + 1]
        if 12_000 <= i < 12_128 or i % 1777 == 0:  # wide rows: span the whole vector
            col[a:b] = rng.integers(0, n_cols, size=b - a)
        else:
            lo = int(max(0, centers[i] - 1500))
            col[a:b] = rng.integers(lo, min(n_cols, lo + 3000), size=b - a)
    return n_cols, off, col


def mixed_phases(dtype):
    """(n_cols, off, col, val, x): blocks of narrow-band rows interleaved with wide rows, empty rows and a window that jumps
    backwards -- ring phases, restarts and global-gather phases in one K1r plan (tests/test_ring_gpu.py)."""
    n_cols, off, col = mixed_phases_pattern()
    rng = np.random.default_rng(199)
    val = rng.uniform(-1, 1, size=len(col)).astype(dtype)
    x = rng.uniform(-1, 1, size=n_cols).astype(dtype)
    return n_cols, off, col, val, x


def _from_lengths(lens, n_cols, dtype, seed):
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lens) + 1, np.uint32)
    np.cumsum(np.asarray(lens, np.int64), out=off[1:])
    col = rng.integers(0, n_cols, int(off[-1]), dtype=np.uint32)
    return n_cols, off, col, rng.uniform(-1, 1, len(col)).astype(dtype)


def merge_long_row_in_scattered(dtype):
    """scattered(40 000) with a row of 7000 entries put in after row 20 000: the row crosses three tile boundaries, so the fix-up folds
    three carries for it.  The seed of its data is one of the draws (about one in four per value type) at which folding the
    three in descending order rounds differently from the kernel's ascending order, in f32 and in f64."""
    off, col, val = scattered(40_000, dtype)
    n, at = 40_000, 20_000
    rng = np.random.default_rng(7014)
    k = int(off[at + 1])
    new_col = rng.integers(0, n, 7000, dtype=np.uint32)
    new_val = rng.uniform(-1, 1, 7000).astype(dtype)
    off64 = off.astype(np.int64)
    off2 = np.concatenate([off64[:at + 2], off64[at + 1:] + 7000]).astype(np.uint32)
    return n, off2, np.concatenate([col[:k], new_col, col[k:]]), np.concatenate([val[:k], new_val, val[k:]])


def merge_arrowhead(dtype):
    return (8000,) + arrowhead(8000, dtype)


def merge_one_row(dtype):
    """one row of 5001 entries (nnz mod 4 == 1: as borrowed arrays the last chunk is read entry by entry)"""
    return _from_lengths([5001], 6000, dtype, 5001)


def merge_empty_stretch(dtype):
    """1000 rows of 0 ... 11 entries, 2500 empty rows (more than a tile of row ends alone), 1000 rows again"""
    rng = np.random.default_rng(2500)
    lens = np.concatenate([rng.integers(0, 12, 1000), np.zeros(2500, np.int64), rng.integers(0, 12, 1000)])
    return _from_lengths(lens, 3000, dtype, 2501)


def merge_rows_end_on_tiles(dtype):
    """rows of 15, 7 and 7 entries over and over: 32 merge items per three rows, so every tile of 2048 items ends with the end of a
    row and the row it leaves open has no entry in it yet (a carry of +0)"""
    return _from_lengths([15, 7, 7] * 256, 1000, dtype, 32)


def merge_single_tile(dtype):
    return _from_lengths(np.random.default_rng(1).integers(0, 20, 100), 300, dtype, 2)


# name -> (builder, the most tile boundaries a row of it crosses must be at least this)
MERGE_CASES = {
    "scattered-long-row": (merge_long_row_in_scattered, 3),
    "arrowhead": (merge_arrowhead, 1),
    "one-row": (merge_one_row, 2),
    "empty-stretch": (merge_empty_stretch, 0),
    "rows-end-on-tiles": (merge_rows_end_on_tiles, 0),
    "single-tile": (merge_single_tile, 0),
}
MERGE_BORROWED = ("one-row", "empty-stretch")


def merge_crossings(off, tile_items=2048):
    """per row: how many tiles end with the row open, its end still to come (the carries the fix-up folds for it; a tile that ends
    with the end of the row before leaves it open with none of its entries: a carry of +0)"""
    n_rows, nnz = len(off) - 1, int(off[-1])
    n_tiles = (n_rows + nnz + tile_items - 1) // tile_items
    rows, _ = oracle.merge_path_search(off, nnz, np.arange(1, n_tiles, dtype=np.uint64) * tile_items)
    return np.bincount(rows[rows < n_rows].astype(np.int64), minlength=n_rows)


def vector_config_names():
    return [name for name in CONFIGS if name in VECTOR_CONFIG_LANES]


_built = {}


def config_matrix(name, dtype):
    """(n_cols, off, col, val, x) of a CONFIGS entry, built once per (builder, value type)"""
    key = (CONFIGS[name].build, np.dtype(dtype))
    if key not in _built:
        off, col, val = CONFIGS[name].build(dtype)
        n = len(off) - 1
        _built[key] = (n, off, col, val, vector_x(n, dtype, 1000 + n))
    return _built[key]


def lane_cases(dtype):
    """Every product the lane-group tests launch on the device, as (id, lanes, (n_cols, off, col, val, x), tail_from): tail_from is
    None for K1 and for K1r on owned (padded) arrays, nnz & ~3 for K1r on borrowed, unpadded ones."""
    for mod in range(4):
        n_cols, off, col, val = ragged(dtype, mod)
        parts = (n_cols, off, col, val, vector_x(n_cols, dtype))
        for lanes in LANES:
            yield "ragged-nnz%d" % mod, lanes, parts, None
            if mod:
                yield "ragged-nnz%d-tail" % mod, lanes, parts, int(off[-1]) & ~3
    for name in vector_config_names():
        if dtype in CONFIGS[name].dtypes:
            yield name, VECTOR_CONFIG_LANES[name], config_matrix(name, dtype), None
    for lanes in (2, 8):
        yield "mixed-phases", lanes, mixed_phases(dtype), None
