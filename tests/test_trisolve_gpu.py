"""GPU: the level-scheduled sparse triangular solve (csrc/trisolve.hip behind smh_crs_trisolve*) pinned BIT FOR BIT to
tests/trisolve_model.py, f32 and f64, LOWER and UPPER, the stored and the implied diagonal, at every lane-group width; its level
schedule against the model's definition, the launch counts of the single-workgroup walk over small levels, the schedule after
the handle changes, non-finite data by class, and every status.  The matrices are tests/trisolve_cases.py's: the CPU test
test_trisolve_model.py shows that each of them moves a bit under an FMA, a reversed chain or a sum-first order."""
import ctypes as C

import numpy as np
import pytest
import torch

import sparsemat_amd as sm
import trisolve_cases as tc
import trisolve_model as tm
from kernel_forms import same
from sparsemat_amd import _lib

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPES = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]
UPLOS = [tm.LOWER, tm.UPPER]


def handle(off, col, val, validate=True):
    n = len(off) - 1
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val, validate=validate)


def assert_same(got, want, what):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert same(got, want), (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


def status_of(call):
    with pytest.raises(_lib.SparseMatPanic) as e:
        call()
    return e.value.status, str(e.value)


def model_solves(off, col, val, b, uplo):
    plan = tm.Plan(off, col, uplo)
    return plan, {unit: tm.trisolve(off, col, val, b, uplo, unit, plan=plan) for unit in (False, True)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLOS)
@pytest.mark.parametrize("name", tc.NAMES)
def test_levels_and_solves_equal_the_model(gpu, name, uplo, dtype):
    off, col, val, b = tc.system(name, dtype, uplo)
    n = len(b)
    a = handle(off, col, val)
    plan, want = model_solves(off, col, val, b, uplo)
    lv = a.trisolve_levels(uplo)
    assert lv["small_level_rows"] == tc.SMALL_LEVEL_ROWS >= 64
    assert lv["n_levels"] == plan.n_levels and np.array_equal(lv["level_of_row"], plan.level)
    sizes = np.bincount(plan.level, minlength=plan.n_levels)
    assert lv["n_launches"] == tc.launches(sizes, lv["small_level_rows"])  # the rule, on every case; and what it comes to:
    if name == "diagonal":
        assert lv["n_levels"] == 1 and lv["n_launches"] == 1
    if name in ("one", "chain3000", "dense70", "ragged129", "lap24x17"):
        assert sizes.max() <= lv["small_level_rows"] and lv["n_launches"] == 1  # however many levels: one workgroup walks them
    if name == "chain3000":
        assert lv["n_levels"] == 3000
    if name == "lap64x65-rb":
        assert sizes.tolist() == [2080, 2080] and lv["n_launches"] == 2  # a launch per level, several workgroups each
    if name == "switch":  # 50 small levels, one of R + 1 rows, 49 small levels: the switch between the two kernels, both ways
        assert lv["n_levels"] == 100 and sizes.max() == lv["small_level_rows"] + 1 and lv["n_launches"] == 3
    for unit in (False, True):
        assert_same(a.trisolve(b, uplo, unit), want[unit], (name, uplo, "unit" if unit else "non-unit", "host"))
    # device vectors, out of place and in place (x is b)
    bd = sm.DenseVec.from_vec(b)
    assert_same(a.trisolve(bd, uplo).to_numpy(), want[False], (name, uplo, "vec"))
    assert same(bd.to_numpy(), b)
    _lib.check(sm.lib().smh_crs_trisolve_vec(a._h, _lib.UPLO[uplo], _lib.SMH_DIAG_NON_UNIT, bd._h, bd._h))
    assert_same(bd.to_numpy(), want[False], (name, uplo, "in place"))
    assert a.trisolve_levels(uplo)["n_launches"] == lv["n_launches"]  # (the schedule is built once)
    assert n == len(want[False])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLOS)
def test_every_lane_group_width(gpu, uplo, dtype):
    """The dense triangle of 70 rows (rows longer than a wavefront) and the ragged one (every strict length 0 .. 129) at every
    width of the lane group, 1 .. 64: the same bits.  (Without a forced width both run with 64 lanes, the grids with 8, the
    chain with 2, the diagonal with 1: test_levels_and_solves_equal_the_model.)"""
    for name in ("dense70", "ragged129", "lap24x17-rb"):
        off, col, val, b = tc.system(name, dtype, uplo)
        a = handle(off, col, val)
        _, want = model_solves(off, col, val, b, uplo)
        for lanes in (1, 2, 4, 8, 16, 32, 64):
            a.set_vector_lanes(lanes)
            for unit in (False, True):
                assert_same(a.trisolve(b, uplo, unit), want[unit], (name, uplo, lanes, unit))


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_levels_at_every_width(gpu, dtype):
    """... and the per-level kernel (two levels of 2080 rows) at every width."""
    off, col, val, b = tc.system("lap64x65-rb", dtype, tm.LOWER)
    a = handle(off, col, val)
    for uplo in UPLOS:
        _, want = model_solves(off, col, val, b, uplo)
        for lanes in (1, 2, 4, 16, 32, 64):
            a.set_vector_lanes(lanes)
            assert_same(a.trisolve(b, uplo), want[False], (uplo, lanes))


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_and_single(gpu, dtype):
    z = sm.SparseMatCRS.from_raw_parts(0, 0, [0], [], np.zeros(0, dtype))
    for uplo in UPLOS:
        lv = z.trisolve_levels(uplo)
        assert lv["n_levels"] == 0 and lv["n_launches"] == 0 and len(lv["level_of_row"]) == 0
        assert len(z.trisolve(np.zeros(0, dtype), uplo)) == 0
        assert z.trisolve(sm.DenseVec.zeros(0, dtype), uplo, unit_diagonal=True).dim() == 0
    one = handle(*tm.from_rows([[(0, 4.0)]], dtype))
    assert one.trisolve([10.0], tm.UPPER).tolist() == [2.5] and one.trisolve([10.0], tm.LOWER, unit_diagonal=True).tolist() == [10.0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_data_reaches_the_rows_that_depend_on_it(gpu, dtype):
    """NaN, +-Inf and -0 in b, and a zero diagonal value: the model's IEEE arithmetic says which rows they reach; the device agrees
    by class on the non-finite rows (a NaN's sign and payload are not arithmetic) and bit for bit, signed zeros included, on
    the others."""
    off, col, val, b = tc.system("lap24x17", dtype, tm.LOWER)
    n = len(b)
    a = handle(off, col, val)
    for uplo in UPLOS:
        plan = tm.Plan(off, col, uplo)
        for k, special in enumerate((np.nan, np.inf, -np.inf, -0.0)):
            bs = b.copy()
            bs[[5 + k, 200 + 3 * k]] = special
            if special == 0:
                bs[:] = -0.0  # all of b: -0 - (v * -0) keeps or loses its sign as IEEE says
            want = tm.trisolve(off, col, val, bs, uplo, False, plan=plan)
            got = a.trisolve(bs, uplo)
            assert_same(got, want, (uplo, special))
            if special != 0:
                finite = np.isfinite(want)
                assert 0 < finite.sum() < n and np.array_equal(np.isfinite(got), finite)  # some rows reached, some not
                assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want))
            else:
                assert np.array_equal(np.signbit(got), np.signbit(want))
    # a zero diagonal VALUE is not an error: s / 0
    v0 = val.copy()
    pos = tm.diag_positions(off, col)
    v0[pos[[7, 300]]] = [0.0, -0.0]
    a0 = handle(off, col, v0)
    for uplo in UPLOS:
        want = tm.trisolve(off, col, v0, b, uplo, False, plan=tm.Plan(off, col, uplo))
        got = a0.trisolve(b, uplo)
        assert np.isinf(want).any() and np.isfinite(want).any()
        assert_same(got, want, (uplo, "zero diagonal"))
        assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want))


@pytest.mark.parametrize("dtype", DTYPES)
def test_schedule_after_the_handle_changes(gpu, dtype):
    off, col, val, b = tc.system("messy", dtype, tm.LOWER)
    n = len(b)
    a = handle(off, col, val)

    def check(o, c, v, what):
        for uplo in UPLOS:
            plan = tm.Plan(o, c, uplo)
            lv = a.trisolve_levels(uplo)
            assert lv["n_levels"] == plan.n_levels and np.array_equal(lv["level_of_row"], plan.level), what
            assert_same(a.trisolve(b, uplo), tm.trisolve(o, c, v, b, uplo, False, plan=plan), (what, uplo))

    check(off, col, val, "fresh")
    # new values on the same structure: the schedule holds positions only, and stays
    v2 = (val * dtype(1.25)).astype(dtype)
    a.update_values(v2)
    check(off, col, v2, "update_values")
    a.scale(0.5)
    v3 = (v2 * dtype(0.5)).astype(dtype)
    check(off, col, v3, "scale")
    # a values-only apply: add to an entry that exists (its first occurrence takes it)
    r0 = 17
    c0 = int(col[off[r0]])
    k0 = off[r0] + int(np.flatnonzero(col[off[r0]:off[r0 + 1]] == c0)[0])
    a.apply([r0], [c0], np.array([0.375], dtype))
    v4 = v3.copy()
    v4[k0] = v4[k0] + dtype(0.375)
    check(off, col, v4, "values-only apply")
    # a new storage order: positions (the diagonal's among them) move, and which of two stored diagonals comes first may change
    a.sort_rows()
    o5, c5, v5 = a.raw_parts()
    assert not np.array_equal(c5, col)
    check(o5, c5, v5, "sort_rows")
    # an apply that creates an entry: new arrays, a new dependency (row 3 on row 1 / row 1 on row 150), new levels
    for r, c in ((3, 1), (1, 150)):
        if not (c5[o5[r]:o5[r + 1]] == c).any():
            a.apply([r], [c], np.array([0.25], dtype))
    o6, c6, v6 = a.raw_parts()
    assert len(c6) > len(c5)
    check(o6, c6, v6, "apply with new entries")
    assert n == a.n_rows()


def test_statuses(gpu):
    L = sm.lib()
    off, col, val, b = tc.system("lap24x17", F32, tm.LOWER)
    n = len(b)
    a = handle(off, col, val)
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.zeros(n, F32)
    lo, nu = _lib.SMH_TRI_LOWER, _lib.SMH_DIAG_NON_UNIT
    x = np.zeros(n, F32)
    host = lambda m, uplo, diag, bb, xx: L.smh_crs_trisolve(m, uplo, diag, bb.ctypes.data, len(bb), xx.ctypes.data, len(xx))
    # not square
    rect = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 1], np.ones(2, F32))
    assert host(rect._h, lo, nu, b[:2].copy(), x[:2].copy()) == _lib.SMH_ERR_NOT_SQUARE
    assert status_of(lambda: rect.trisolve_levels())[0] == _lib.SMH_ERR_NOT_SQUARE
    assert L.smh_crs_trisolve_vec(rect._h, lo, nu, sm.DenseVec.zeros(2, F32)._h, sm.DenseVec.zeros(2, F32)._h) == _lib.SMH_ERR_NOT_SQUARE
    # dimension mismatch
    assert host(a._h, lo, nu, b[:-1].copy(), x) == _lib.SMH_ERR_DIM_MISMATCH
    assert host(a._h, lo, nu, b, x[:-1].copy()) == _lib.SMH_ERR_DIM_MISMATCH
    assert L.smh_crs_trisolve_vec(a._h, lo, nu, bd._h, sm.DenseVec.zeros(n + 1, F32)._h) == _lib.SMH_ERR_DIM_MISMATCH
    # a stored column >= n (the handle was made without validation)
    wide = sm.SparseMatCRS.from_raw_parts(2, 2, [0, 1, 3], [0, 1, 5], np.ones(3, F32), validate=False)
    assert host(wide._h, lo, nu, b[:2].copy(), x[:2].copy()) == _lib.SMH_ERR_INDEX_RANGE
    assert status_of(lambda: wide.trisolve_levels("upper"))[0] == _lib.SMH_ERR_INDEX_RANGE
    # invalid: NULL pointers, dtype, uplo / diag, partial overlap
    assert L.smh_crs_trisolve(None, lo, nu, b.ctypes.data, n, x.ctypes.data, n) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_trisolve(a._h, lo, nu, None, n, x.ctypes.data, n) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_trisolve(a._h, lo, nu, b.ctypes.data, n, None, n) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_trisolve_vec(a._h, lo, nu, None, xd._h) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_trisolve_vec(a._h, lo, nu, bd._h, None) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_trisolve_vec(None, lo, nu, bd._h, xd._h) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_trisolve_levels(None, lo, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_trisolve_vec(a._h, lo, nu, bd._h, sm.DenseVec.zeros(n, F64)._h) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_trisolve_vec(a._h, lo, nu, sm.DenseVec.zeros(n, F64)._h, xd._h) == _lib.SMH_ERR_INVALID
    for uplo, diag in ((2, nu), (-1, nu), (lo, 2), (lo, -1)):
        assert host(a._h, uplo, diag, b, x) == _lib.SMH_ERR_INVALID
        assert L.smh_crs_trisolve_vec(a._h, uplo, diag, bd._h, xd._h) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_trisolve_levels(a._h, 2, None, None, None, None) == _lib.SMH_ERR_INVALID
    t = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    v0 = sm.DenseVec.from_device_ptr(t.data_ptr(), n, F32, keep=t)
    v1 = sm.DenseVec.from_device_ptr(t.data_ptr() + 16, n, F32, keep=t)
    assert L.smh_crs_trisolve_vec(a._h, lo, nu, v0._h, v1._h) == _lib.SMH_ERR_INVALID and "overlap" in sm.lib().smh_last_error().decode()
    both = np.zeros(n + 4, F32)
    assert L.smh_crs_trisolve(a._h, lo, nu, both.ctypes.data, n, both.ctypes.data + 8, n) == _lib.SMH_ERR_INVALID
    # a handle that holds an orphaned entry (the first push of a replay into a SparseMatCRS)
    orphaned = sm.SparseMatCRS.from_triplets([1, 0, 1, 0], [1, 0, 0, 1], np.ones(4, F32), into_crs=True)
    assert orphaned.orphans() == 1 and orphaned.n_rows() == orphaned.n_cols() == 2
    assert host(orphaned._h, lo, nu, b[:2].copy(), x[:2].copy()) == _lib.SMH_ERR_INVALID and "orphan" in sm.lib().smh_last_error().decode()
    assert status_of(lambda: orphaned.trisolve_levels())[0] == _lib.SMH_ERR_INVALID
    # NON_UNIT without a stored diagonal names the first such row; UNIT needs none
    o, c, v = tm.from_rows([[(0, 2.0)], [(0, 1.0), (1, 2.0)], [(1, 1.0)], [(3, 1.0)], [(0, 1.0)]], F32)
    nd = handle(o, c, v)
    st, msg = status_of(lambda: nd.trisolve(np.ones(5, F32)))
    assert st == _lib.SMH_ERR_INVALID and "row 2" in msg
    assert_same(nd.trisolve(np.ones(5, F32), unit_diagonal=True), tm.trisolve(o, c, v, np.ones(5, F32), tm.LOWER, True), "unit, no diagonal")
    # nothing above has left the good handle unusable
    assert_same(a.trisolve(b), tm.trisolve(off, col, val, b, tm.LOWER, False, plan=tm.Plan(off, col, tm.LOWER)), "after the refusals")
