"""GPU: the factorized sparse approximate inverse (smh_crs_fsai: csrc/fsai.hip), its application (smh_crs_fsai_apply_vec) and its CG
(smh_pcg_fsai_solve*, csrc/pcg.hip) pinned BIT FOR BIT to tests/fsai_model.py: G, G^T (offsets, columns, values) and not_spd on the
cases of tests/fsai_cases.py (which tests/test_fsai_model.py shows to move a bit under each wrong variant), at every lane width and
on both sides of the LDS-to-scratch switch (fsai_cases.fit(lanes)); the refusals and statuses; the application against the device's
own products of g and gt, each held to the suite's parity bound first; and x, the number of entered bodies and f64(r.r) of the
solver with the model fed by those products and the matrix's, as tests/test_ilu_gpu.py does for ILU(0)."""
import ctypes as C
import math

import numpy as np
import pytest

import fsai_cases as fc
import fsai_model as fm
import sgs_model as sg
import sparsemat_amd as sm
import trisolve_model as tm
from kernel_forms import same
from sparsemat_amd import _lib
from test_sgs_gpu import BIG_PATH, SMALL_PATHS, assert_result, check_path, device_product, is_fused, path_ids, path_system

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPES = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]


def handle(off, col, val, validate=True):
    n = len(off) - 1
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val, validate=validate)


def status_of(call):
    with pytest.raises(_lib.SparseMatPanic) as e:
        call()
    return e.value.status, str(e.value)


def assert_factor(g, gt, want, what, by_class=False):
    """g and gt against the model's (goff, gcol, gval): offsets and columns equal, values bit for bit (by_class: bits where the
    model is finite, the class elsewhere); gt is the model's transposition and what the device's own transposition of g gives."""
    goff, gcol, gval = want
    n = len(goff) - 1
    for h, (o, c, v), name in ((g, (goff, gcol, gval), "g"), (gt, fm.transpose(goff, gcol, gval), "gt")):
        ho, hc, hv = h.raw_parts()
        assert h.n_rows() == n and h.dtype == gval.dtype and (n == 0 or h.n_cols() == n), (what, name)
        assert np.array_equal(ho, o) and np.array_equal(hc, c), (what, name, "pattern")
        if by_class:
            fin = np.isfinite(v)
            assert same(hv[fin], v[fin]) and np.array_equal(np.isnan(hv), np.isnan(v)) and np.array_equal(hv[np.isinf(v)], v[np.isinf(v)]), (what, name)
        else:
            bad = np.flatnonzero(hv != v)
            assert same(hv, v), (what, name, len(bad), bad[:5], hv[bad[:5]], v[bad[:5]])
    if n > 1:  # (n = 1: gt is a copy of g, where the one-operation transposition would leave an orphan)
        to, tcol, tv = g.transpose().raw_parts()
        ho, hc, hv = gt.raw_parts()
        assert np.array_equal(to, ho) and np.array_equal(tcol, hc) and same(tv, hv), (what, "the device's own transposition")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(fc.NAMES))
def test_factor_equals_the_model(gpu, name, dtype):
    off, col, val = fc.matrix(name, dtype)
    goff, gcol, gval, want_bad = fc.factor(name, dtype)
    a = handle(off, col, val)
    g, gt, bad = a.fsai()
    assert bad is None and want_bad is None
    assert_factor(g, gt, (goff, gcol, gval), name)
    assert same(a.raw_parts()[2], val)  # (the matrix itself is untouched)
    lens = np.diff(goff.astype(np.int64))
    if name == "dense128" or name == "arrow128":
        assert lens.max() == fc.MAX_ROW
    if len(lens) and name not in ("one", "two"):  # which form a case runs in (the lanes are the mean row's)
        long_rows = (lens > fc.fit(fc.auto_lanes(goff))).sum()
        assert (long_rows > 0) == (name in ("dense70", "dense128", "ragged", "arrow128")), (name, long_rows)
        assert long_rows < len(lens)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ragged", "dense70", "table2", "lap3d12"])
def test_every_lane_width_gives_the_same_bits(gpu, name, dtype):
    """ragged has every m from 1 to 70 four times: for every lane width L the rows of m = L, L + 1 and 2 L + 1 (one, two and three
    trips of the group over the triangle's rows) and of m = fit(L) and fit(L) + 1 (the last row in the LDS, the first in scratch)."""
    off, col, val = fc.matrix(name, dtype)
    goff, gcol, gval, _ = fc.factor(name, dtype)
    lens = set(np.diff(goff.astype(np.int64)).tolist())
    a = handle(off, col, val)
    for lanes in fc.LANES:
        if name == "ragged":
            assert {lanes, lanes + 1, min(2 * lanes + 1, 70), fc.fit(lanes), fc.fit(lanes) + 1} <= lens
        a.set_vector_lanes(lanes)
        g, gt, bad = a.fsai()
        assert bad is None
        assert_factor(g, gt, (goff, gcol, gval), (name, lanes))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(fc.REFUSED))
def test_rows_beyond_the_limit_are_refused(gpu, name, dtype):
    a = handle(*fc.matrix(name, dtype))
    st, msg = status_of(a.fsai)
    assert st == _lib.SMH_ERR_INVALID and "row %d " % fc.REFUSED[name] in msg and str(fc.MAX_ROW) in msg
    g, gt, bad = C.c_void_p(), C.c_void_p(), C.c_size_t(7)
    assert sm.lib().smh_crs_fsai(a._h, C.byref(g), C.byref(gt), C.byref(bad)) == _lib.SMH_ERR_INVALID
    assert g.value is None and gt.value is None and bad.value == 7


@pytest.mark.parametrize("dtype", DTYPES)
def test_not_spd_and_non_finite_values(gpu, dtype):
    # a block [[1, 2], [2, 1]] in rows 2 and 3 of a diagonal matrix: the last pivot of row 3 is 1 - 2 * 2 = -3; row 5's is negative too
    rows = [[(0, 4.0)], [(1, 9.0)], [(2, 1.0), (3, 2.0)], [(2, 2.0), (3, 1.0)], [(4, 16.0)], [(4, 0.5), (5, -1.0)]]
    off, col, val = tm.from_rows(rows, dtype)
    want = fm.fsai(off, col, val)
    g, gt, bad = handle(off, col, val).fsai()
    assert bad == want[3] == 3 and np.isnan(want[2][3:5]).all() and np.isnan(want[2][-2:]).all()
    assert_factor(g, gt, want[:3], "not spd", by_class=True)
    assert g.raw_parts()[2][:3].tolist() == [0.5, float(dtype(1) / dtype(3)), 1.0] and g.raw_parts()[2][5] == 0.25
    # a zero pivot: 1 / sqrt(0) is +Inf, and the row is reported
    g, _, bad = handle(*tm.from_rows([[(0, 1.0)], [(1, 0.0)]], dtype)).fsai()
    assert bad == 1 and g.raw_parts()[2].tolist() == [1.0, np.inf]
    # a stored NaN and a stored Inf: bits where the model is finite, the class elsewhere
    off, col, val = fc.matrix("table1", dtype)
    val = val.copy()
    pos = tm.diag_positions(off, col)
    val[pos[40] - 1] = np.nan
    val[pos[200]] = np.inf
    want = fm.fsai(off, col, val)
    assert 2 < (~np.isfinite(want[2])).sum() < 40 and np.isnan(want[2]).any()
    for lanes in (0, 1, 64):
        a = handle(off, col, val)
        if lanes:
            a.set_vector_lanes(lanes)
        g, gt, bad = a.fsai()
        assert bad == want[3] and bad is not None
        assert_factor(g, gt, want[:3], ("non-finite", lanes), by_class=True)


def test_statuses(gpu):
    L = sm.lib()

    def refused(a):
        g, gt, bad = C.c_void_p(), C.c_void_p(), C.c_size_t(7)
        st = L.smh_crs_fsai(a._h, C.byref(g), C.byref(gt), C.byref(bad))
        assert g.value is None and gt.value is None and bad.value == 7  # nothing is made
        return st, L.smh_last_error().decode()

    st, msg = refused(handle(*tm.from_rows([[(0, 1.0)], [(1, 1.0)], [(2, 1.0), (0, 1.0)], [(3, 1.0), (1, 1.0)]], F32)))
    assert st == _lib.SMH_ERR_INVALID and "row 2" in msg and "ascending" in msg
    st, msg = refused(handle(*tm.from_rows([[(0, 1.0)], [(0, 1.0), (1, 1.0), (1, 1.0)]], F32)))
    assert st == _lib.SMH_ERR_INVALID and "row 1" in msg and "ascending" in msg
    st, msg = refused(handle(*tm.from_rows([[(0, 1.0)], [(1, 1.0)], [(0, 1.0)], [(0, 1.0), (2, 1.0)]], F32)))
    assert st == _lib.SMH_ERR_INVALID and "row 2" in msg and "diagonal" in msg
    orphan = sm.SparseMatCRS.from_triplets([1, 0, 1, 0], [1, 0, 0, 1], np.ones(4, F32), into_crs=True)
    assert orphan.orphans() == 1
    st, msg = refused(orphan)
    assert st == _lib.SMH_ERR_INVALID and "orphan" in msg
    rect = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 1], np.ones(2, F32))
    assert refused(rect)[0] == _lib.SMH_ERR_NOT_SQUARE
    wide = sm.SparseMatCRS.from_raw_parts(2, 2, [0, 1, 3], [0, 1, 5], np.ones(3, F32), validate=False)
    assert refused(wide)[0] == _lib.SMH_ERR_INDEX_RANGE
    # the order of the contract: not square before unsorted
    both = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 2, 3], [1, 0, 1], np.ones(3, F32))
    assert refused(both)[0] == _lib.SMH_ERR_NOT_SQUARE
    # NULL pointers; not_spd_out may be NULL
    good = handle(*fc.matrix("table3", F32))
    g, gt, bad = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert L.smh_crs_fsai(None, C.byref(g), C.byref(gt), C.byref(bad)) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_fsai(good._h, None, C.byref(gt), C.byref(bad)) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_fsai(good._h, C.byref(g), None, C.byref(bad)) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_fsai(good._h, C.byref(g), C.byref(gt), None) == _lib.SMH_OK and g.value and gt.value
    gm, gtm = sm.SparseMatCRS(g, F32), sm.SparseMatCRS(gt, F32)
    assert_factor(gm, gtm, fc.factor("table3", F32)[:3], "not_spd_out NULL")
    # the application's statuses
    n = good.n_rows()
    r, z = sm.DenseVec.zeros(n, F32), sm.DenseVec.zeros(n, F32)
    for args in ((None, gtm._h, r._h, z._h), (gm._h, None, r._h, z._h), (gm._h, gtm._h, None, z._h), (gm._h, gtm._h, r._h, None)):
        assert L.smh_crs_fsai_apply_vec(*args) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_fsai_apply_vec(gm._h, gtm._h, r._h, sm.DenseVec.zeros(n, F64)._h) == _lib.SMH_ERR_INVALID
    assert status_of(lambda: gm.fsai_apply(gtm, np.zeros(n - 1, F32)))[0] == _lib.SMH_ERR_DIM_MISMATCH
    assert status_of(lambda: rect.fsai_apply(gtm, np.zeros(2, F32)))[0] == _lib.SMH_ERR_NOT_SQUARE
    small = handle(*fc.matrix("two", F32))
    assert status_of(lambda: gm.fsai_apply(small, np.zeros(n, F32)))[0] == _lib.SMH_ERR_DIM_MISMATCH
    g64 = handle(*[x if i < 2 else x.astype(F64) for i, x in enumerate(gtm.raw_parts())])
    assert status_of(lambda: gm.fsai_apply(g64, np.zeros(n, F32)))[0] == _lib.SMH_ERR_INVALID
    assert status_of(lambda: orphan.fsai_apply(orphan, np.zeros(2, F32)))[0] == _lib.SMH_ERR_INVALID


def test_empty_one_and_two(gpu):
    for dtype in (F32, F64):
        z = handle(*fc.matrix("empty", dtype))
        g, gt, bad = z.fsai()
        assert g.n_rows() == 0 and gt.n_rows() == 0 and g.n_non_zero_entries() == 0 and bad is None and len(g.fsai_apply(gt, np.zeros(0, dtype))) == 0
        s = sm.FSAIConjugateGradient(1e-6, 10)
        s.solve(z, np.zeros(0, dtype), np.zeros(0, dtype))
        assert s.iterations == 1  # (the empty r.r is 0: the first body's stop test passes, as SGS-PCG's)
        g, gt, bad = handle(*tm.from_rows([[(0, 4.0)]], dtype)).fsai()
        assert g.raw_parts()[2].tolist() == [0.5] and gt.raw_parts()[2].tolist() == [0.5] and bad is None
        assert g.fsai_apply(gt, [10.0]).tolist() == [2.5]
        # tridiag(2, -1) of 2 rows: row 1 is (1, 2) / sqrt(6) before the scaling by hand
        g, gt, bad = handle(*tm.from_rows([[(0, 2.0), (1, -1.0)], [(0, -1.0), (1, 2.0)]], dtype)).fsai()
        T = dtype
        gg = T(1) / np.sqrt(T(1.5))
        assert same(g.raw_parts()[2], np.array([T(1) / np.sqrt(T(2)), T(0.5) * gg, gg], dtype)) and bad is None


# ---- the application ----------------------------------------------------------------------------------------------------------
def checked_apply(g, gt, gp, gtp):
    """r -> G^T (G r) by the device's own AUTO products of g and gt, each held to the parity bound against its raw parts."""
    first, second = device_product(g, "auto", *gp), device_product(gt, "auto", *gtp)
    return lambda r: second(first(r))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["table1", "table2-rb", "dense70", "lap3d12", "nonsymmetric"])
def test_apply_equals_the_products(gpu, name, dtype):
    off, col, val = fc.matrix(name, dtype)
    goff, gcol, gval, _ = fc.factor(name, dtype)
    n = len(off) - 1
    g, gt, _ = handle(off, col, val).fsai()
    r = tm.awkward(np.random.default_rng(n), n, dtype)
    want = checked_apply(g, gt, (goff, gcol, gval), fm.transpose(goff, gcol, gval))(r)
    assert np.isfinite(want).all() and want.any()
    got = g.fsai_apply(gt, r)
    assert same(got, want), np.flatnonzero(got != want)[:5]
    rd = sm.DenseVec.from_vec(r)
    assert same(g.fsai_apply(gt, rd).to_numpy(), want) and same(rd.to_numpy(), r)  # out of place
    assert g.fsai_apply(gt, rd, out=rd) is rd and same(rd.to_numpy(), want)        # in place: z may be r
    # the factor handles are ordinary ones
    assert same(g.clone().raw_parts()[2], gval)
    rows = np.arange(n, dtype=np.uint32)
    assert same(np.asarray(g.get_many(rows, rows)), gval[goff[1:].astype(np.int64) - 1])


# ---- FSAI-PCG ------------------------------------------------------------------------------------------------------------------
_SYSTEMS = {}


def system(k, ordering):
    """table case k and its model factor (G and G^T as raw parts), computed once"""
    if (k, ordering) not in _SYSTEMS:
        off, col, val, b, tol = sg.table_case(k, ordering)
        goff, gcol, gval, bad = fc.factor("table%d%s" % (k, "-rb" if ordering == "red_black" else ""), val.dtype)
        assert bad is None
        _SYSTEMS[k, ordering] = off, col, val, b, tol, (goff, gcol, gval), fm.transpose(goff, gcol, gval)
    return _SYSTEMS[k, ordering]


def run_host(m, factor, b, x0, tol, iter_max, variant):
    s = sm.FSAIConjugateGradient(tol, iter_max, variant=variant)
    x = x0.copy()
    s.solve(m, b, x, factor=factor)
    return x, s.iterations, np.float64(s.r_norm_squared)


def run_vec(m, factor, b, x0, tol, iter_max, variant, check_every):
    s = sm.FSAIConjugateGradient(tol, iter_max, factor=factor, variant=variant, check_every=check_every)
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x0)
    s.solve(m, bd, xd)
    assert same(bd.to_numpy(), b)
    return xd.to_numpy(), s.iterations, np.float64(s.r_norm_squared)


@pytest.mark.parametrize("variant", ["stream", "seq", "auto"])
@pytest.mark.parametrize("ordering", ["natural", "red_black"])
@pytest.mark.parametrize("k", range(len(sg.TABLE)))
def test_solve_equals_the_model_fed_by_the_device_products(gpu, k, ordering, variant):
    """To the table's tolerance from x0 = 0: the body count, x and r.r of the model; the residual of the solution; factor=None (the
    solver factors the matrix itself) gives the bits of a passed pair.  On the device too the count stays under 0.6 of Jacobi's."""
    off, col, val, b, tol, gp, gtp = system(k, ordering)
    n = len(b)
    a = handle(off, col, val)
    a.prepare(variant)
    g, gt, bad = a.fsai()
    assert bad is None
    assert_factor(g, gt, gp, (k, ordering))
    x0 = np.zeros(n, val.dtype)
    want = sg.sgs_pcg(off, col, val, b, x0, tol, 500, fused=is_fused(a, variant), product=device_product(a, variant, off, col, val),
                      precond=checked_apply(g, gt, gp, gtp))
    assert 10 < want.iterations < 120 and math.sqrt(want.r_norm_squared) < tol
    assert_result(run_host(a, (g, gt), b, x0, tol, 500, variant), want, (k, ordering, variant, "host"))
    assert_result(run_vec(a, (g, gt), b, x0, tol, 500, variant, 3), want, (k, ordering, variant, "vec/3"))
    own = sm.FSAIConjugateGradient(tol, 500, variant=variant)
    x = x0.copy()
    own.solve(a, b, x)
    assert same(x, want.x) and own.iterations == want.iterations and own.not_spd is None and same(own.factor[0].raw_parts()[2], gp[2])
    # the true residual: the recurrence's r drifts from b - A x by at most a few u |A| |x| per body
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(off.astype(np.int64))), col.astype(np.int64)] = val.astype(F64)
    u = 2.0 ** (-24 if val.dtype == F32 else -53)
    drift = 8 * want.iterations * u * (np.abs(A) @ np.abs(x.astype(F64)) + np.abs(b)).max() * math.sqrt(n)
    assert np.linalg.norm(A @ x.astype(F64) - b.astype(F64)) < tol + drift
    if variant == "auto":
        jac = sm.JacobiConjugateGradient(tol, 2000)
        jac.solve(a, b, x0.copy())
        assert want.iterations <= 0.6 * jac.iterations, (want.iterations, jac.iterations)


@pytest.mark.parametrize("dtype", DTYPES)
def test_stops_batches_and_iter_max(gpu, dtype):
    """From a random x0 with tol = 0 and iter_max = 11 (an iter_max inside a batch of 3, of 8 and of the host default; check_every
    1, 3 and 8), then stops on tol inside a replayed batch and on a batch boundary, each twice on the same handles; iter_max = 0."""
    k = 3 if dtype == F32 else 1
    off, col, val, b, _, gp, gtp = system(k, "red_black")
    n = len(b)
    a = handle(off, col, val)
    g, gt, _ = a.fsai()
    f = (g, gt)
    x0 = np.random.default_rng(7).uniform(-1, 1, n).astype(dtype)
    product, precond = device_product(a, "stream", off, col, val), checked_apply(g, gt, gp, gtp)
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


def path_factor(off, col, val):
    """(g, gt, the model's preconditioner fed by their products) of a path system, from a handle of its own: the build is
    deterministic, so the factor of check_path's handle has these bits (asserted where it is made)."""
    g, gt, bad = handle(off, col, val).fsai()
    assert bad is None
    return g, gt, checked_apply(g, gt, g.raw_parts(), gt.raw_parts())


def check_fsai_path(case, dtype, model_factor):
    off, col, val, _, _ = path_system(*case[:4], dtype)
    g, gt, precond = path_factor(off, col, val)
    if model_factor:
        want = fm.fsai(off, col, val)
        assert want[3] is None
        assert_factor(g, gt, want[:3], case)
    made = {}

    def factor_of(a):
        if id(a) not in made:
            g2, gt2, _ = a.fsai()
            assert all(same(x, y) if x.dtype.kind == "f" else np.array_equal(x, y) for x, y in zip(g2.raw_parts() + gt2.raw_parts(), g.raw_parts() + gt.raw_parts()))
            made[id(a)] = (g2, gt2)
        return made[id(a)]
    check_path(case, dtype, precond, lambda a, *args: run_host(a, factor_of(a), *args), lambda a, *args: run_vec(a, factor_of(a), *args))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", SMALL_PATHS, ids=path_ids(SMALL_PATHS))
def test_bits_at_every_path_size(gpu, case, dtype):
    """tests/test_sgs_gpu.py's small path sizes (n = 3 and n = 391: no whole vector, a tail of 1 and of 3, two workgroups, a replayed
    batch and one body more) with the FSAI pair."""
    check_fsai_path(case, dtype, True)


def test_bits_on_a_second_trip_of_the_grid(gpu):
    """n = 262 447 in f64: the sweeps' threads make a second trip.  The factor is the device's (its bits are the cases' business),
    the model is fed by the checked products of its raw parts."""
    check_fsai_path(BIG_PATH, F64, False)


def test_the_class_factors_by_itself_and_refuses_a_matrix_that_is_not_spd(gpu):
    off, col, val = tm.from_rows([[(0, 1.0), (1, 2.0)], [(0, 2.0), (1, 1.0)]], F64)
    a = handle(off, col, val)
    s = sm.FSAIConjugateGradient(1e-8, 10)
    x = np.zeros(2)
    with pytest.raises(ValueError, match="row 1"):
        s.solve(a, np.ones(2), x)
    assert s.not_spd == 1 and not x.any()
    # a passed pair is the caller's business: the solve runs on it (NaN in, NaN out, no error)
    g, gt, bad = a.fsai()
    assert bad == 1
    s.solve(a, np.ones(2), x, factor=(g, gt))
    assert s.not_spd is None and s.iterations == 10 and np.isnan(x).all()


def test_solver_statuses(gpu):
    L = sm.lib()
    off, col, val, b, tol, gp, gtp = system(3, "natural")
    n = len(b)
    a = handle(off, col, val)
    g, gt, _ = a.fsai()
    x = np.zeros(n, F32)
    solver = sm.FSAIConjugateGradient(tol, 50)
    two = handle(*fc.matrix("two", F32)).fsai()
    g64 = handle(gp[0], gp[1], gp[2].astype(F64))
    rect = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 1], np.ones(2, F32))
    orphan = sm.SparseMatCRS.from_triplets([1, 0, 1, 0], [1, 0, 0, 1], np.ones(4, F32), into_crs=True)
    bd = sm.DenseVec.from_vec(b)
    for factor, status in (((two[0], gt), _lib.SMH_ERR_DIM_MISMATCH), ((g, two[1]), _lib.SMH_ERR_DIM_MISMATCH), ((g64, gt), _lib.SMH_ERR_INVALID),
                           ((g, g64), _lib.SMH_ERR_INVALID), ((rect, gt), _lib.SMH_ERR_NOT_SQUARE), ((g, rect), _lib.SMH_ERR_NOT_SQUARE)):
        assert status_of(lambda: solver.solve(a, b, x, factor=factor))[0] == status
        xd = sm.DenseVec.zeros(n, F32)
        assert status_of(lambda: solver.solve(a, bd, xd, factor=factor))[0] == status
        assert not xd.to_numpy().any()
    two_a = handle(*fc.matrix("two", F32))
    st, msg = status_of(lambda: solver.solve(two_a, np.ones(2, F32), np.zeros(2, F32), factor=(orphan, two[1])))
    assert st == _lib.SMH_ERR_INVALID and "orphan" in msg and "FSAI" in msg
    assert status_of(lambda: solver.solve(rect, np.ones(2, F32), np.zeros(2, F32), factor=(g, gt)))[0] == _lib.SMH_ERR_NOT_SQUARE
    assert status_of(lambda: solver.solve(a, b[:-1], x, factor=(g, gt)))[0] == _lib.SMH_ERR_DIM_MISMATCH
    assert status_of(lambda: solver.solve(a, bd, sm.DenseVec.zeros(n - 1, F32), factor=(g, gt)))[0] == _lib.SMH_ERR_DIM_MISMATCH
    wide = sm.SparseMatCRS.from_raw_parts(n, n, gp[0], np.where(np.arange(len(gp[1])) == 5, n + 3, gp[1]).astype(np.uint32), gp[2], validate=False)
    assert status_of(lambda: solver.solve(a, b, x, factor=(wide, gt)))[0] == _lib.SMH_ERR_INDEX_RANGE
    assert not x.any()
    # invalid arguments of the raw entry points
    xd = sm.DenseVec.zeros(n, F32)
    host = lambda *h: L.smh_pcg_fsai_solve(*h, b.ctypes.data, n, x.ctypes.data, n, 1e-6, 10, 0, None, None)
    assert host(None, g._h, gt._h) == host(a._h, None, gt._h) == host(a._h, g._h, None) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_fsai_solve(a._h, g._h, gt._h, None, n, x.ctypes.data, n, 1e-6, 10, 0, None, None) == _lib.SMH_ERR_INVALID
    vec = lambda *h: L.smh_pcg_fsai_solve_vec(*h, 1e-6, 10, 0, 0, None, None)
    assert vec(None, g._h, gt._h, bd._h, xd._h) == vec(a._h, None, gt._h, bd._h, xd._h) == vec(a._h, g._h, None, bd._h, xd._h) == _lib.SMH_ERR_INVALID
    assert vec(a._h, g._h, gt._h, None, xd._h) == vec(a._h, g._h, gt._h, bd._h, bd._h) == _lib.SMH_ERR_INVALID
    assert vec(a._h, g._h, gt._h, bd._h, sm.DenseVec.zeros(n, F64)._h) == _lib.SMH_ERR_INVALID
    assert not x.any() and not xd.to_numpy().any()
    # the output pointers may be NULL, and the good pair still solves
    assert L.smh_pcg_fsai_solve_vec(a._h, g._h, gt._h, bd._h, xd._h, tol, 50, 0, 0, None, None) == _lib.SMH_OK
    want = sg.sgs_pcg(off, col, val, b, x, tol, 50, fused=is_fused(a, "auto"), product=device_product(a, "auto", off, col, val),
                      precond=checked_apply(g, gt, gp, gtp))
    assert same(xd.to_numpy(), want.x)
