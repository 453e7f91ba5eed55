"""CG (cg.hip), Jacobi-PCG (pcg.hip) and BiCGSTAB (bicgstab.hip) pinned BIT FOR BIT through every product kernel family, each in
the form it is named for (asserted through the handle's own getters, before and after the solves): x, the number of entered
bodies, f64(r.r) and BiCGSTAB's breakdown code equal tests/cg_model.py / tests/bicgstab_model.py in "device" mode, the model
taking every product -- the initial residual's included -- from the DEVICE's eager product of the same variant on the same
handle (device_product), which is held to the suite's parity bound against the oracle (util.assert_spmv_close) before the
model may use it.  So the model is never anchored to the code under test alone, and no tolerance appears in this file.

The statement per case: x0 random, tol = 0, iter_max = 11; check_every = 4 on the DenseVec entry points (three replays of the
captured batch, the last body a no-op) and the default on the host entry points (CG 4; PCG and BiCGSTAB 8: one replay and three
plain launches); each solve twice on the same handle (the second captures its graph anew).  For one value type per
configuration also a stop on tol in the middle of a batch (stop_tolerance).  The premise -- three eager products of one x and
one replayed from a graph captured on a side stream have the same bytes -- is asserted first on every matrix here.

The matrices (all square, symmetric in their non-zero values, strictly diagonally dominant with a positive diagonal: SPD;
off-diagonal values in (-1, 0), a_ii = 1 + sum_j |a_ij|):
  band(n, w, L)    row i holds the diagonal and 15 pairs i -+ d (the same 15 offsets d <= w in every row, 1 and w among them),
                   ascending; columns that fall off the matrix are replaced by stored 0.0 at unused columns next to the
                   diagonal, so every row has L = 31 entries, or 32 with one more stored zero (all 16-byte chunks row-aligned)
  scattered(n)     4 random pairs per row (about 9 entries with the diagonal), every 997th row and column about 3000 more
                   (hubs = False: none), rows stored in random order
  arrowhead(n)     40 hub rows and columns of about 2000 entries, 2 random pairs in every row (about 15 entries with the hub
                   columns), stored in random order
  stencil7(g)      the 7-point pattern of oracle.laplace3d(*g) with non-constant coefficients
  laplace3d(24^3)  the oracle's constant-coefficient Laplacian (two distinct values: K1s XD-V's dictionary)
The shapes are the smallest at which each form engages; what the getters must report is in CONFIGS.  The final numbers:
band(20 000, 4000, 31 | 32) for K1 and the single-window K1r forms; band(48 000, 10 000, 32) for the 32 768-column ring (at 30 000
rows the 16 384-column ring still serves 53 % of the rows and the plan keeps it); stencil7(130 x 130 x 6) for the banded ring (a
48 x 48 x 24 grid fits one window); scattered(40 000) for merge (316 tiles), K2c (5 blocks of 8192 columns) and K2t (3 slices),
without its hubs for K2f; arrowhead(8000) for K2s (40 long rows); 24^3 for K1s (the stage forced: x is under 1 MB)."""
import contextlib
import functools
import math
import os

import numpy as np
import pytest
import torch

import bicgstab_model as bm
import cg_model
import oracle
import sparsemat_amd as sm
from util import assert_spmv_close

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ITER_MAX = 11
CHECK_EVERY = 4


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
CASES = [pytest.param(name, dt, id="%s-%s" % (name, "f32" if dt == F32 else "f64")) for name, c in CONFIGS.items() for dt in c.dtypes]


# ---- the device's product, checked -------------------------------------------------------------------------------------------
def device_product(m, variant, off, col, val):
    """product(v) = m.mvp(v, variant) computed eagerly on the device, handed on only after util.assert_spmv_close has held it to the
    parity bound against the oracle's product.  (A vector met before is answered from the first, checked, product: the stop
    cases walk the same iterates again.)"""
    seen = {}

    def product(v):
        v = np.ascontiguousarray(v, val.dtype)
        key = v.tobytes()
        if key not in seen:
            y = m.mvp(v, variant=variant)
            assert_spmv_close(y, off, col, val, v, "solver product, variant %s" % variant)
            seen[key] = y
        return seen[key].copy()
    return product


def assert_products_reproducible(m, variant, x):
    """Three eager products of x and one replayed from a graph captured on a side stream: the same bytes."""
    first = m.mvp(x, variant=variant)
    for _ in range(2):
        assert m.mvp(x, variant=variant).tobytes() == first.tobytes(), "eager products of one x differ"
    xt = torch.from_numpy(x).cuda()
    yt = torch.zeros(m.n_rows(), dtype=xt.dtype, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            m.mvp_dev(xt.data_ptr(), len(x), yt.data_ptr(), variant, stream=side.cuda_stream)
    yt.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert yt.cpu().numpy().tobytes() == first.tobytes(), "the product replayed from a graph differs from the eager one"


# ---- the solvers -------------------------------------------------------------------------------------------------------------
def same(a, b):
    """bit equality (any NaN equals any NaN: its sign and payload are not arithmetic)"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def run_host(solver, a, b, x0):
    x = x0.copy()
    solver.solve(a, b, x)
    return x


def run_vec(solver, a, b, x0):
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x0)
    solver.solve(a, bd, xd)
    assert same(bd.to_numpy(), b)  # (b is read only)
    return xd.to_numpy()


class Solver:
    """One of the three: the model, the device solves (entry point by entry point) and what is compared."""

    def __init__(self, name):
        self.name = name

    def model(self, off, col, val, b, x0, tol, iter_max, product, fused):
        if self.name == "bicgstab":
            return bm.bicgstab(off, col, val, b, x0, tol, iter_max, product=product)
        return (cg_model.cg if self.name == "cg" else cg_model.pcg)(off, col, val, b, x0, tol, iter_max, fused=fused, product=product)

    def device(self, a, b, x0, tol, iter_max, variant):
        """[(entry point, x, (iterations, f64(rr)[, breakdown, converged]))]"""
        out = []
        if self.name == "pcg":
            runs = [("host", sm.JacobiConjugateGradient(tol, iter_max, variant=variant), run_host)]
        else:
            cls = sm.ConjugateGradient if self.name == "cg" else sm.BiCGStab
            runs = [("vec/%d" % CHECK_EVERY, cls(tol, iter_max, variant=variant, check_every=CHECK_EVERY), run_vec),
                    ("host", cls(tol, iter_max, variant=variant), run_host)]
        for what, s, run in runs:
            x = run(s, a, b, x0)
            scalars = (s.iterations, np.float64(s.r_norm_squared))
            if self.name == "bicgstab":
                scalars += (s.breakdown, s.converged)
            out.append((what, x, scalars))
        return out

    def scalars(self, want):
        if self.name == "bicgstab":
            return want.iterations, np.float64(want.r_norm_squared), want.breakdown, want.converged
        return want.iterations, np.float64(want.r_norm_squared)

    def events(self, want):
        """the norms the stop tests of the bodies saw, in order: [(body, norm)] (BiCGSTAB: the half step's, then the full step's)"""
        if self.name == "bicgstab":
            ev = []
            for k, (ss, rr) in enumerate(zip(want.ss_list, want.rr_list)):
                ev += [(k + 1, math.sqrt(float(ss))), (k + 1, math.sqrt(float(rr)))]
            return ev
        return [(k + 1, math.sqrt(float(rr))) for k, rr in enumerate(want.rr_list)]


SOLVERS = [Solver("cg"), Solver("pcg"), Solver("bicgstab")]


def assert_same_result(solver, got, want, what):
    entry, x, scalars = got
    assert np.isfinite(x).all(), (what, entry, "x is not finite")
    w = solver.scalars(want)
    assert scalars[0] == w[0], (what, entry, "iterations", scalars[0], w[0])
    assert same(scalars[1], w[1]), (what, entry, "r.r", scalars[1], w[1])
    assert scalars[2:] == w[2:], (what, entry, "breakdown, converged", scalars[2:], w[2:])
    bad = np.flatnonzero(x != want.x)
    assert same(x, want.x), (what, entry, "x", len(bad), bad[:5], x[bad[:5]], want.x[bad[:5]])


def stop_tolerance(solver, want):
    """(body k, tol): tol lies strictly between the norm a stop test of body k sees and the smallest norm any earlier stop test
    saw, so the loop has to leave in body k, neither sooner nor later -- k in the middle of a batch of 4 (and of 8)."""
    ev = solver.events(want)
    for k in (6, 7, 10, 3, 2):
        for e, (body, norm) in enumerate(ev):
            if body == k and e and norm < 0.9 * min(v for _, v in ev[:e]):  # (a gap far wider than any rounding of the square root)
                return k, 0.5 * (norm + min(v for _, v in ev[:e]))
    raise AssertionError(("no body in the middle of a batch undercuts all earlier norms", ev))


@pytest.mark.parametrize("name,dtype", CASES)
def test_solvers_equal_the_model_fed_by_the_checked_device_product(gpu, name, dtype):
    cfg = CONFIGS[name]
    off, col, val = cfg.build(dtype)
    n = len(off) - 1
    assert n < 131_072  # (the models' reduction trees at these sizes are pinned by test_cg_bits_gpu.py / test_bicgstab_gpu.py)
    rng = np.random.default_rng(1000 + n)
    b, x0 = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
    a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    fused_env = dict(SMH_CG_FUSED_DOT=None, SMH_STREAM_RPT=None) if cfg.fused else {}
    with env(**cfg.env, **fused_env):
        cfg.knobs(a)
        a.prepare(cfg.variant)
        cfg.check(a)
        assert_products_reproducible(a, cfg.variant, x0)
        product = device_product(a, cfg.variant, off, col, val)
        for solver in SOLVERS:
            want = solver.model(off, col, val, b, x0, 0.0, ITER_MAX, product, cfg.fused)
            assert want.iterations == ITER_MAX and np.isfinite(want.x).all()
            for attempt in ("first solve", "second solve"):
                got = solver.device(a, b, x0, 0.0, ITER_MAX, cfg.variant)
                for g in got:
                    assert_same_result(solver, g, want, (name, solver.name, attempt))
            if cfg.same_as:
                for g in solver.device(a, b, x0, 0.0, ITER_MAX, cfg.same_as):
                    assert_same_result(solver, g, want, (name, solver.name, "as " + cfg.same_as))
            if dtype == cfg.stop or len(cfg.dtypes) == 1:
                k, tol = stop_tolerance(solver, want)
                stopped = solver.model(off, col, val, b, x0, tol, 50, product, cfg.fused)
                assert stopped.iterations == k and not same(stopped.x, solver.model(off, col, val, b, x0, 0.0, k - 1, product, cfg.fused).x)
                for g in solver.device(a, b, x0, tol, 50, cfg.variant):
                    assert_same_result(solver, g, stopped, (name, solver.name, "stop in body %d" % k))
        cfg.check(a)  # (the solves have changed no form)
