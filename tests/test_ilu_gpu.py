"""GPU: the ILU(0) factorization (smh_crs_ilu0, smh_crs_ilu0_refactor: csrc/ilu.hip), its application (smh_crs_ilu_apply_vec) and
its CG (smh_pcg_ilu_solve*, csrc/pcg.hip) pinned BIT FOR BIT to tests/ilu_model.py: the factor's values and zero_pivot on the
cases of tests/ilu_cases.py (which tests/test_ilu_model.py shows to move a bit under an FMA, a reversed row and a late division),
at every lane width, across the long-row switch (ilu_cases.SLICE * lanes entries) and the two launch kinds; the statuses; and x,
the number of entered bodies and f64(r.r) of the solver with the model fed by the device's own product, as tests/test_sgs_gpu.py
does for SGS."""
import ctypes as C
import math

import numpy as np
import pytest

import ilu_cases as ic
import ilu_model as im
import sgs_model as sg
import sparsemat_amd as sm
import trisolve_cases as tc
import trisolve_model as tm
from kernel_forms import env, same
from sparsemat_amd import _lib
from test_sgs_gpu import SMALL_PATHS, assert_result, check_path, device_product, is_fused, path_ids, path_system
from util import assert_spmv_close

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPES = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]
LANES = (1, 2, 4, 8, 16, 32, 64)


def handle(off, col, val, validate=True):
    n = len(off) - 1
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val, validate=validate)


def values(m):
    return m.raw_parts()[2]


def status_of(call):
    with pytest.raises(_lib.SparseMatPanic) as e:
        call()
    return e.value.status, str(e.value)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(ic.NAMES))
def test_factor_equals_the_model(gpu, name, dtype):
    off, col, val = ic.matrix(name, dtype)
    want, want_zp = ic.factor(name, dtype)
    a = handle(off, col, val)
    f, zp = a.ilu0()
    o, c, got = f.raw_parts()
    assert np.array_equal(o, off) and np.array_equal(c, col) and f.dtype == a.dtype
    bad = np.flatnonzero(got != want)
    assert same(got, want), (name, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    assert zp == want_zp and zp is None
    assert same(values(a), val)  # (the matrix itself is untouched)
    # the schedule is the LOWER one of the pattern: its launches are the factorization's
    lv = f.trisolve_levels("lower")
    sizes = np.bincount(tm.levels(off, col, tm.LOWER)[0]) if len(off) > 1 else np.zeros(0, np.int64)
    assert lv["small_level_rows"] == ic.SMALL_LEVEL_ROWS and lv["n_launches"] == tc.launches(sizes, ic.SMALL_LEVEL_ROWS)
    if name == "chain3000":
        assert lv["n_levels"] == 3000 and lv["n_launches"] == 1  # one workgroup walks them
    if name == "switch":
        assert lv["n_launches"] == 3
    if name == "grid130x131":  # small levels, then 129, 130, 130, 129 rows on a grid each, then small levels
        assert sizes.max() == 130 and lv["n_launches"] == 6
    if name.endswith("-rb"):
        assert lv["n_levels"] == 2 and lv["n_launches"] == 2 and sizes.min() > ic.SMALL_LEVEL_ROWS  # the grid launch
    if name.startswith("arrow"):
        assert lv["n_levels"] == 2 and np.diff(off.astype(np.int64)).max() == 5001 > ic.SLICE * 64  # a long row at any width


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["dense70", "ragged131", "ragged290", "arrow_last", "arrow_first", "table2", "random2000"])
def test_every_lane_width_gives_the_same_bits(gpu, name, dtype):
    """The long-row switch is at ilu_cases.SLICE * lanes entries: ragged131 (rows of 1 .. 133 entries) has rows on both sides of it
    for 1 to 32 lanes, ragged290 (.. 291) for 64 as well; a row of n entries is one pass of L lanes for n <= L, two for n <= 2 L."""
    off, col, val = ic.matrix(name, dtype)
    want, _ = ic.factor(name, dtype)
    lens = np.diff(off.astype(np.int64))
    a = handle(off, col, val)
    for lanes in LANES:
        if name.startswith("ragged"):
            switch = ic.SLICE * lanes
            assert (lens.max() > switch and lens.min() <= switch) == (name == "ragged290" or lanes <= 32)
            assert name != "ragged131" or {lanes, lanes + 1, 2 * lanes, 2 * lanes + 1} <= set(lens.tolist())
        a.set_vector_lanes(lanes)
        f, zp = a.ilu0()
        got = values(f)
        bad = np.flatnonzero(got != want)
        assert same(got, want) and zp is None, (name, lanes, len(bad), bad[:5])


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_pivot_and_non_finite_values(gpu, dtype):
    f, zp = handle(*tm.from_rows([[(0, 1), (1, 1)], [(0, 1), (1, 1)]], dtype)).ilu0()
    assert values(f).tolist() == [1, 1, 1, 0] and zp == 1
    # the zero pivot is divided by: IEEE's values, no error, the first such row reported
    off, col, val = tm.from_rows([[(0, 1), (1, 1)], [(0, 1), (1, 1), (2, 1)], [(1, 1), (2, 1)], [(3, 0.0)]], dtype)
    f, zp = handle(off, col, val).ilu0()
    want, want_zp = im.ilu0(off, col, val)
    assert zp == want_zp == 1 and same(values(f), want) and values(f).tolist() == [1, 1, 1, 0, 1, np.inf, -np.inf, 0]
    # a stored NaN and a stored Inf: bits where the model is finite, the class elsewhere
    off, col, val = ic.matrix("table1", dtype)
    val = val.copy()
    pos = tm.diag_positions(off, col)
    val[pos[40] + 1] = np.nan
    val[pos[200]] = np.inf
    want, want_zp = im.ilu0(off, col, val, vector=True)
    for lanes in (0, 1, 64):
        a = handle(off, col, val)
        if lanes:
            a.set_vector_lanes(lanes)
        f, zp = a.ilu0()
        got = values(f)
        fin = np.isfinite(want)
        assert 10 < (~fin).sum() < len(want) and np.isnan(want).any() and zp == want_zp
        assert same(got[fin], want[fin]) and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)])


def test_statuses(gpu):
    L = sm.lib()
    f32 = F32
    good = handle(*ic.matrix("table3", f32))
    # an unsorted row, a duplicate, a missing diagonal: the first such row named; nothing is made
    st, msg = status_of(lambda: handle(*tm.from_rows([[(0, 1.0)], [(1, 1.0)], [(2, 1.0), (0, 1.0)], [(3, 1.0), (1, 1.0)]], f32)).ilu0())
    assert st == _lib.SMH_ERR_INVALID and "row 2" in msg and "ascending" in msg
    st, msg = status_of(lambda: handle(*tm.from_rows([[(0, 1.0)], [(0, 1.0), (1, 1.0), (1, 1.0)]], f32)).ilu0())
    assert st == _lib.SMH_ERR_INVALID and "row 1" in msg and "ascending" in msg
    st, msg = status_of(lambda: handle(*tm.from_rows([[(0, 1.0)], [(1, 1.0)], [(0, 1.0)], [(0, 1.0), (2, 1.0)]], f32)).ilu0())
    assert st == _lib.SMH_ERR_INVALID and "row 2" in msg and "diagonal" in msg
    unsorted = handle(*tm.from_rows([[(1, 1.0), (0, 4.0)], [(1, 4.0), (0, 1.0)]], f32))
    assert status_of(unsorted.ilu0)[0] == _lib.SMH_ERR_INVALID
    unsorted.sort_rows()  # (the way there)
    assert values(unsorted.ilu0()[0]).tolist() == [4.0, 1.0, 0.25, 3.75]
    # an orphan, not square, a column beyond n
    orphan = sm.SparseMatCRS.from_triplets([1, 0, 1, 0], [1, 0, 0, 1], np.ones(4, f32), into_crs=True)
    assert orphan.orphans() == 1 and orphan.n_rows() == orphan.n_cols() == 2
    st, msg = status_of(orphan.ilu0)
    assert st == _lib.SMH_ERR_INVALID and "orphan" in msg
    rect = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 1], np.ones(2, f32))
    assert status_of(rect.ilu0)[0] == _lib.SMH_ERR_NOT_SQUARE
    wide = sm.SparseMatCRS.from_raw_parts(2, 2, [0, 1, 3], [0, 1, 5], np.ones(3, f32), validate=False)
    assert status_of(wide.ilu0)[0] == _lib.SMH_ERR_INDEX_RANGE
    # NULL pointers; zero_pivot_out may be NULL
    h, zp = C.c_void_p(), C.c_size_t()
    assert L.smh_crs_ilu0(None, C.byref(h), C.byref(zp)) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_ilu0(good._h, None, C.byref(zp)) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_ilu0(good._h, C.byref(h), None) == _lib.SMH_OK and h.value
    f = sm.SparseMatCRS(h, f32)
    assert same(values(f), ic.factor("table3", f32)[0])
    assert L.smh_crs_ilu0_refactor(None, good._h, None) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_ilu0_refactor(f._h, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_ilu0_refactor(f._h, good._h, None) == _lib.SMH_OK
    n = good.n_rows()
    r, z = sm.DenseVec.zeros(n, f32), sm.DenseVec.zeros(n, f32)
    assert L.smh_crs_ilu_apply_vec(None, r._h, z._h) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_ilu_apply_vec(f._h, None, z._h) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_ilu_apply_vec(f._h, r._h, sm.DenseVec.zeros(n, F64)._h) == _lib.SMH_ERR_INVALID
    assert status_of(lambda: f.ilu_apply(np.zeros(n - 1, f32)))[0] == _lib.SMH_ERR_DIM_MISMATCH
    assert status_of(lambda: rect.ilu_apply(np.zeros(2, f32)))[0] == _lib.SMH_ERR_NOT_SQUARE


@pytest.mark.parametrize("dtype", DTYPES)
def test_refactor(gpu, dtype):
    """New values on the same pattern: after scale and after update_values the refactored handle equals a fresh factorization (and
    the model); another pattern, size or dtype is refused and leaves the factor as it was."""
    off, col, val = ic.matrix("random2000", dtype)
    a = handle(off, col, val)
    f, _ = a.ilu0()
    x = tm.awkward(np.random.default_rng(5), len(off) - 1, dtype)
    f.mvp(x)  # (a value-derived form may exist by now: the refactorization drops it)
    a.scale(0.37)
    scaled = values(a)
    assert f.ilu0_refactor(a) is None
    assert same(values(f), values(a.ilu0()[0])) and same(values(f), im.ilu0(off, col, scaled, vector=True)[0])
    assert_spmv_close(f.mvp(x), off, col, values(f), x, "the factor's own product after a refactorization")
    new = val.copy()
    new[tm.diag_positions(off, col)] *= 1.5
    a.update_values(new)
    assert f.ilu0_refactor(a) is None
    want = im.ilu0(off, col, new, vector=True)[0]
    assert same(values(f), want) and same(values(a.ilu0()[0]), want)
    # a zero pivot shows in a refactorization as in a factorization
    o2, c2, v2 = tm.from_rows([[(0, 1), (1, 1)], [(0, 1), (1, 2)]], dtype)
    a2 = handle(o2, c2, v2)
    f2, zp = a2.ilu0()
    assert zp is None and values(f2).tolist() == [1, 1, 1, 1]
    a2.update_values(np.array([1, 1, 1, 1], dtype))
    assert f2.ilu0_refactor(a2) == 1 and values(f2).tolist() == [1, 1, 1, 0]
    # refused: another pattern with the same n and nnz (one column moved), another nnz, another n, another dtype, itself
    c3 = col.copy()
    row = next(i for i in range(len(off) - 1) if col[off[i + 1] - 1] < len(off) - 2 and off[i + 1] - off[i] > 1)
    c3[off[row + 1] - 1] += 1
    for other, status in ((handle(off, c3, new), _lib.SMH_ERR_INVALID), (handle(*ic.matrix("table2", dtype)), _lib.SMH_ERR_DIM_MISMATCH),
                          (handle(*im.random_pattern(2000, dtype, seed=10)), _lib.SMH_ERR_INVALID),
                          (handle(off, col, new.astype(F32 if dtype == F64 else F64)), _lib.SMH_ERR_INVALID), (f, _lib.SMH_ERR_INVALID)):
        assert status_of(lambda: f.ilu0_refactor(other))[0] == status
        assert same(values(f), want)
    unsorted = handle(*tm.from_rows([[(1, 1.0), (0, 4.0)], [(1, 4.0), (0, 1.0)]], dtype))
    assert status_of(lambda: f2.ilu0_refactor(unsorted))[0] == _lib.SMH_ERR_INVALID and values(f2).tolist() == [1, 1, 1, 0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["table1", "table2-rb", "random2000", "dense70"])
def test_apply_and_the_factor_as_a_handle(gpu, name, dtype):
    """z = U^-1 L^-1 r bit for bit, numpy and DenseVec, out of place and in place; the factor is an ordinary handle: its product
    and its triangular solves are those of its values."""
    off, col, val = ic.matrix(name, dtype)
    w, _ = ic.factor(name, dtype)
    n = len(off) - 1
    f, _ = handle(off, col, val).ilu0()
    r = tm.awkward(np.random.default_rng(n), n, dtype)
    plans = (tm.Plan(off, col, tm.LOWER), tm.Plan(off, col, tm.UPPER))
    want = im.ilu_apply(off, col, w, r, plans)
    assert same(want, im.ilu_apply(off, col, w, r)) and np.isfinite(want).all()
    got = f.ilu_apply(r)
    assert same(got, want), np.flatnonzero(got != want)[:5]
    rd = sm.DenseVec.from_vec(r)
    assert same(f.ilu_apply(rd).to_numpy(), want) and same(rd.to_numpy(), r)
    _lib.check(sm.lib().smh_crs_ilu_apply_vec(f._h, rd._h, rd._h))  # z may be r
    assert same(rd.to_numpy(), want)
    assert same(f.trisolve(r, "lower", unit_diagonal=True), tm.trisolve(off, col, w, r, tm.LOWER, True, plan=plans[0]))
    assert same(f.trisolve(r, "upper"), tm.trisolve(off, col, w, r, tm.UPPER, False, plan=plans[1]))
    assert_spmv_close(f.mvp(r), off, col, w, r, "the factor's own product")
    # L U z = r to the substitutions' backward error: gamma_(d + 2) per row of each, d its strict entries (tests/test_sgs_model.py)
    L, U = im.dense_factors(off, col, w)
    u = 2.0 ** (-24 if dtype == F32 else -53)
    depth = max(tm.row_depth(off, col, tm.LOWER), tm.row_depth(off, col, tm.UPPER))
    bound = 1.1 * 3 * (depth + 2) * u * (np.abs(L) @ np.abs(U)) @ np.abs(want.astype(F64))
    assert (np.abs(L @ (U @ want.astype(F64)) - r.astype(F64)) <= bound).all()


def test_empty_and_single(gpu):
    for dtype in (F32, F64):
        z = handle(*ic.matrix("empty", dtype))
        f, zp = z.ilu0()
        assert f.n_rows() == 0 and zp is None and len(f.ilu_apply(np.zeros(0, dtype))) == 0 and f.ilu0_refactor(z) is None
        s = sm.ILUConjugateGradient(1e-6, 10)
        s.solve(z, np.zeros(0, dtype), np.zeros(0, dtype))
        assert s.iterations == 1  # (the empty r.r is 0: the first body's stop test passes, as SGS-PCG's)
        one = handle(*tm.from_rows([[(0, 4.0)]], dtype))
        f, zp = one.ilu0()
        assert values(f).tolist() == [4.0] and zp is None and f.ilu_apply([10.0]).tolist() == [2.5]
        f0, zp = handle(*tm.from_rows([[(0, 0.0)]], dtype)).ilu0()
        assert zp == 0 and values(f0).tolist() == [0.0]


# ---- ILU(0)-PCG -------------------------------------------------------------------------------------------------------------
_SYSTEMS = {}


def system(k, ordering):
    """table case k, its model factor and the model's preconditioner, computed once"""
    if (k, ordering) not in _SYSTEMS:
        off, col, val, b, tol = sg.table_case(k, ordering)
        w, zp = im.ilu0(off, col, val, vector=True)
        assert zp is None
        plans = (tm.Plan(off, col, tm.LOWER), tm.Plan(off, col, tm.UPPER))
        _SYSTEMS[k, ordering] = off, col, val, b, tol, w, (lambda r: im.ilu_apply(off, col, w, r, plans))
    return _SYSTEMS[k, ordering]


def run_host(m, f, b, x0, tol, iter_max, variant):
    s = sm.ILUConjugateGradient(tol, iter_max, variant=variant)
    x = x0.copy()
    s.solve(m, b, x, factor=f)
    return x, s.iterations, np.float64(s.r_norm_squared)


def run_vec(m, f, b, x0, tol, iter_max, variant, check_every):
    s = sm.ILUConjugateGradient(tol, iter_max, variant=variant, check_every=check_every)
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x0)
    s.solve(m, bd, xd, factor=f)
    assert same(bd.to_numpy(), b)
    return xd.to_numpy(), s.iterations, np.float64(s.r_norm_squared)


@pytest.mark.parametrize("variant", ["stream", "seq", "auto"])
@pytest.mark.parametrize("ordering", ["natural", "red_black"])
@pytest.mark.parametrize("k", range(len(sg.TABLE)))
def test_solve_equals_the_model_fed_by_the_device_product(gpu, k, ordering, variant):
    """To the table's tolerance from x0 = 0: the body count, x and r.r of the model; the residual of the solution; factor=None
    (the solver factors the matrix itself) gives the bits of a passed factor.  On the device too the count stays under 0.6 of
    plain CG's, and under SGS-PCG's in the natural ordering."""
    off, col, val, b, tol, w, precond = system(k, ordering)
    n = len(b)
    a = handle(off, col, val)
    a.prepare(variant)
    f, _ = a.ilu0()
    assert same(values(f), w)
    x0 = np.zeros(n, val.dtype)
    product = device_product(a, variant, off, col, val)
    want = sg.sgs_pcg(off, col, val, b, x0, tol, 500, fused=is_fused(a, variant), product=product, precond=precond)
    assert 10 < want.iterations < 120 and math.sqrt(want.r_norm_squared) < tol
    assert_result(run_host(a, f, b, x0, tol, 500, variant), want, (k, ordering, variant, "host"))
    assert_result(run_vec(a, f, b, x0, tol, 500, variant, 3), want, (k, ordering, variant, "vec/3"))
    own = sm.ILUConjugateGradient(tol, 500, variant=variant)
    x = x0.copy()
    own.solve(a, b, x)
    assert same(x, want.x) and own.iterations == want.iterations and own.zero_pivot is None and same(values(own.factor), w)
    # the true residual: the recurrence's r drifts from b - A x by at most a few u |A| |x| per body
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(off.astype(np.int64))), col.astype(np.int64)] = val.astype(F64)
    u = 2.0 ** (-24 if val.dtype == F32 else -53)
    drift = 8 * want.iterations * u * (np.abs(A) @ np.abs(x.astype(F64)) + np.abs(b)).max() * math.sqrt(n)
    assert np.linalg.norm(A @ x.astype(F64) - b.astype(F64)) < tol + drift
    if variant == "auto":
        cg, sgs = sm.ConjugateGradient(tol, 2000), sm.SGSConjugateGradient(tol, 2000)
        cg.solve(a, b, x0.copy())
        sgs.solve(a, b, x0.copy())
        assert want.iterations < 0.6 * cg.iterations, (want.iterations, cg.iterations)
        if ordering == "natural":
            assert want.iterations < sgs.iterations, (want.iterations, sgs.iterations)


@pytest.mark.parametrize("dtype", DTYPES)
def test_stops_batches_and_iter_max(gpu, dtype):
    """From a random x0 with tol = 0 and iter_max = 11 (an iter_max inside a batch of 3, of 8 and of the host default; check_every
    1, 3 and 8), then stops on tol inside a replayed batch and on a batch boundary, each twice on the same handles; iter_max = 0."""
    k = 3 if dtype == F32 else 1
    off, col, val, b, _, w, precond = system(k, "red_black")
    n = len(b)
    a = handle(off, col, val)
    f, _ = a.ilu0()
    x0 = np.random.default_rng(7).uniform(-1, 1, n).astype(dtype)
    product = device_product(a, "stream", off, col, val)
    model = lambda tol, iter_max: sg.sgs_pcg(off, col, val, b, x0, tol, iter_max, fused=True, product=product, precond=precond)
    want = model(0.0, 11)
    assert want.iterations == 11 and np.isfinite(want.x).all()
    for attempt in range(2):
        assert_result(run_host(a, f, b, x0, 0.0, 11, "stream"), want, ("iter_max", "host", attempt))
        for ce in (1, 3, 8):
            assert_result(run_vec(a, f, b, x0, 0.0, 11, "stream", ce), want, ("iter_max", ce, attempt))
    norms = [math.sqrt(float(v)) for v in want.rr_list]
    kinds = set()
    for body in range(4, 11):
        before = min(norms[:body - 1])
        if not norms[body - 1] < 0.95 * before:
            continue
        tol = 0.5 * (norms[body - 1] + before)
        stopped = model(tol, 50)
        assert stopped.iterations == body and not same(stopped.x, model(0.0, body - 1).x)
        for ce in (1, 3, 8):
            for attempt in range(2):
                assert_result(run_vec(a, f, b, x0, tol, 50, "stream", ce), stopped, ("stop", body, ce, attempt))
            if ce > 1:
                kinds.add("boundary" if body % ce == 0 else "inside")
        assert_result(run_host(a, f, b, x0, tol, 50, "stream"), stopped, ("stop", body, "host"))
    assert kinds == {"boundary", "inside"}, (kinds, norms)
    none = model(0.0, 0)
    assert_result(run_host(a, f, b, x0, 0.0, 0, "stream"), none, "iter_max 0")
    assert_result(run_vec(a, f, b, x0, 0.0, 0, "stream", 3), none, "iter_max 0, vec")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", SMALL_PATHS, ids=path_ids(SMALL_PATHS))
def test_bits_at_every_path_size(gpu, case, dtype):
    """tests/test_sgs_gpu.py's small path sizes (n = 3 and n = 391: no whole vector, a tail of 1 and of 3, two workgroups, a replayed
    batch and one body more) with the ILU(0) factor.  The second trip of the grid is SGS's case alone: the kernels are the same ones."""
    off, col, val, _, _ = path_system(*case[:4], dtype)
    w, zp = im.ilu0(off, col, val, vector=True)
    assert zp is None
    plans = (tm.Plan(off, col, tm.LOWER), tm.Plan(off, col, tm.UPPER))
    made = {}

    def factor_of(a):
        if id(a) not in made:
            made[id(a)] = a.ilu0()[0]
            assert same(values(made[id(a)]), w)
        return made[id(a)]
    check_path(case, dtype, lambda r: im.ilu_apply(off, col, w, r, plans),
               lambda a, *args: run_host(a, factor_of(a), *args), lambda a, *args: run_vec(a, factor_of(a), *args))


@pytest.mark.parametrize("dtype", DTYPES)
def test_node_budget_changes_no_bit(gpu, dtype):
    """The red-black 64 x 65 grid: 2 launches per solve.  With the budget of a captured batch lowered to 40 nodes
    (SMH_SGS_GRAPH_NODES) batches of 8 bodies become batches of 2; lowered to 8 a single body is beyond it and the loop runs
    uncaptured.  Both give the bits of the replayed route."""
    off, col, val = sg.lap2d(64, 65, dtype, seed=2, spread=1.0)
    off, col, val = sg.permute_symmetric(off, col, val, sg.red_black(64, 65))
    n = len(off) - 1
    a = handle(off, col, val)
    f, _ = a.ilu0()
    w, _ = im.ilu0(off, col, val, vector=True)
    assert same(values(f), w) and f.trisolve_levels("lower")["n_launches"] == 2 and f.trisolve_levels("upper")["n_launches"] == 2
    plans = (tm.Plan(off, col, tm.LOWER), tm.Plan(off, col, tm.UPPER))
    precond = lambda r: im.ilu_apply(off, col, w, r, plans)
    rng = np.random.default_rng(3)
    b, x0 = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
    product = device_product(a, "stream", off, col, val)
    want = sg.sgs_pcg(off, col, val, b, x0, 0.0, 13, fused=True, product=product, precond=precond)
    norms = [math.sqrt(float(v)) for v in want.rr_list]
    body = next(j for j in range(5, 13) if norms[j - 1] < 0.95 * min(norms[:j - 1]))
    tol = 0.5 * (norms[body - 1] + min(norms[:body - 1]))
    stopped = sg.sgs_pcg(off, col, val, b, x0, tol, 50, fused=True, product=product, precond=precond)
    assert stopped.iterations == body
    for nodes in (None, "40", "8"):
        with env(SMH_SGS_GRAPH_NODES=nodes):
            assert_result(run_vec(a, f, b, x0, 0.0, 13, "stream", 8), want, ("budget", nodes))
            assert_result(run_vec(a, f, b, x0, tol, 50, "stream", 8), stopped, ("budget, stop", nodes))
            assert_result(run_host(a, f, b, x0, tol, 50, "stream"), stopped, ("budget, host", nodes))


def test_solver_statuses(gpu):
    L = sm.lib()
    off, col, val, b, tol, w, precond = system(3, "natural")
    n = len(b)
    a = handle(off, col, val)
    f, _ = a.ilu0()
    x = np.zeros(n, F32)
    solver = sm.ILUConjugateGradient(tol, 50)
    # a zero and an absent diagonal entry in the factor: refused, the row named
    pos = tm.diag_positions(off, col)
    w0 = w.copy()
    w0[pos[37]] = 0.0
    st, msg = status_of(lambda: solver.solve(a, b, x, factor=handle(off, col, w0)))
    assert st == _lib.SMH_ERR_INVALID and "row 37" in msg and "ILU" in msg
    keep = np.ones(len(col), bool)
    keep[pos[[41, 99]]] = False
    o2 = np.zeros(n + 1, np.uint32)
    o2[1:] = np.cumsum(np.add.reduceat(keep.astype(np.int64), off[:-1].astype(np.int64)))
    nodiag = handle(o2, col[keep], w[keep])
    st, msg = status_of(lambda: solver.solve(a, b, x, factor=nodiag))
    assert st == _lib.SMH_ERR_INVALID and "row 41" in msg
    st, msg = status_of(lambda: nodiag.ilu_apply(b))
    assert st == _lib.SMH_ERR_INVALID and "row 41" in msg
    assert not x.any()
    # a and f differ in n or dtype; not square; vector sizes
    small = handle(*ic.matrix("dense70", F32)).ilu0()[0]
    assert status_of(lambda: solver.solve(a, b, x, factor=small))[0] == _lib.SMH_ERR_DIM_MISMATCH
    assert status_of(lambda: solver.solve(a, sm.DenseVec.from_vec(b), sm.DenseVec.zeros(n, F32), factor=small))[0] == _lib.SMH_ERR_DIM_MISMATCH
    f64 = handle(off, col, w.astype(F64))
    assert status_of(lambda: solver.solve(a, b, x, factor=f64))[0] == _lib.SMH_ERR_INVALID
    rect = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 1], np.ones(2, F32))
    assert status_of(lambda: solver.solve(rect, np.ones(2, F32), np.zeros(2, F32), factor=f))[0] == _lib.SMH_ERR_NOT_SQUARE
    assert status_of(lambda: solver.solve(a, b[:-1], x, factor=f))[0] == _lib.SMH_ERR_DIM_MISMATCH
    assert status_of(lambda: solver.solve(a, sm.DenseVec.from_vec(b), sm.DenseVec.zeros(n - 1, F32), factor=f))[0] == _lib.SMH_ERR_DIM_MISMATCH
    assert not x.any()
    # invalid arguments of the raw entry points
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.zeros(n, F32)
    assert L.smh_pcg_ilu_solve(None, f._h, b.ctypes.data, n, x.ctypes.data, n, 1e-6, 10, 0, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_ilu_solve(a._h, None, b.ctypes.data, n, x.ctypes.data, n, 1e-6, 10, 0, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_ilu_solve(a._h, f._h, None, n, x.ctypes.data, n, 1e-6, 10, 0, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_ilu_solve_vec(a._h, f._h, None, xd._h, 1e-6, 10, 0, 0, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_ilu_solve_vec(a._h, None, bd._h, xd._h, 1e-6, 10, 0, 0, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_ilu_solve_vec(a._h, f._h, bd._h, bd._h, 1e-6, 10, 0, 0, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_ilu_solve_vec(a._h, f._h, bd._h, sm.DenseVec.zeros(n, F64)._h, 1e-6, 10, 0, 0, None, None) == _lib.SMH_ERR_INVALID
    # the output pointers may be NULL, and the good pair still solves
    assert L.smh_pcg_ilu_solve_vec(a._h, f._h, bd._h, xd._h, tol, 50, 0, 0, None, None) == _lib.SMH_OK
    want = sg.sgs_pcg(off, col, val, b, x, tol, 50, fused=is_fused(a, "auto"), product=device_product(a, "auto", off, col, val), precond=precond)
    assert same(xd.to_numpy(), want.x)
