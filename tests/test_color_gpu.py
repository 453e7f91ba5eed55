"""GPU: the multicolour ordering of csrc/color.hip (smh_crs_color) -- colors, perm, n_colors and n_rounds exactly the numpy model
of its definition (tests/color_model.py), f32 and f64 handles, seeds 0 and 1; then what it is for: the level schedule, the
triangular solves and SGS-PCG on the matrix it permutes.

The fixed constants of the kernels, each with cases on both sides (tests/color_model.py names the cases):
  * kColorThreadDeg = 32: a vertex of up to 32 neighbours is walked by one thread, a longer list by its workgroup
    (hubs_around_the_thread_limit: degrees 31, 32, 33 and 300; the star's hub has 5000; the cliques are all walked by workgroups,
    the grids, chains and leaves all by threads);
  * kColorBlock = 256, the lane width: worklist vertices per workgroup and sweep (worklist_255 / _256 / _257: one workgroup with
    an idle lane, a full one, two workgroups) and the lanes that walk a long list together (hubs_around_the_block: degrees 255,
    256, 257 -- one pass with an idle lane, one full pass, two passes);
  * kColorWindow = 64 colours per mask: clique_63 and clique_64 stay inside the first window (colours up to 62 / 63), clique_65
    fills it and moves the base once, clique_130 twice;
  * kColorGrid * kColorBlock = 4096 * 256 = 1048576 worklist vertices per sweep of a round (worklist_grid_cap_minus_1 / _cap /
    _plus_1: stars of 1048575, 1048576 and 1048577 vertices -- one sweep short of full, one full sweep, a second sweep of one
    vertex; about a second each, most of it the model);
  * kColorFirstBatch = 4 rounds before the first read-back, doubling to 64: single, isolated_5 and the stars end inside the
    first batch (rounds enqueued after the last vertex do nothing), path_5 at seed 1 on its last round, the grids (10 to 24
    rounds) in the second and the third batch, comb_70 (70 rounds at seed 0, more than 4 + 8 + 16 + 32) in the fifth; the cliques (63 .. 130 rounds) cross
    four and five batch boundaries with ONE vertex coloured per round."""
import ctypes as C
import math

import numpy as np
import pytest

import color_model as cm
import reorder_model as rm
import sgs_model as sg
import sparsemat_amd as sm
import trisolve_model as tm
from kernel_forms import same
from sparsemat_amd import _lib
from util import assert_spmv_close

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
NAMES = sorted(cm.CASES)


def device_product(m, variant, off, col, val):
    """the device's own product of that variant, held to the suite's parity bound against the oracle (tests/test_sgs_gpu.py's)"""
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


def is_fused(m, variant):
    return variant == "stream" or (variant == "auto" and m.resolved_variant()[0] == "stream")


def handle(n, off, col, dtype=F32, val=None):
    val = np.ones(len(col), dtype) if val is None else val
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)


def assert_equals_model(got, want, what):
    perm, stats = got
    assert perm.dtype == np.uint32 and stats["colors"].dtype == np.uint32
    assert (stats["n_colors"], stats["n_rounds"]) == (want["n_colors"], want["n_rounds"]), what
    assert np.array_equal(stats["colors"], want["colors"]), (what, "first difference at %d" % int(np.argmax(stats["colors"] != want["colors"])))
    assert np.array_equal(perm, want["perm"]), what
    assert np.array_equal(stats["color_counts"], want["color_counts"]), what


@pytest.mark.parametrize("name", NAMES)
def test_equals_the_model(gpu, name):
    n, off, col = cm.case(name)
    rng = np.random.default_rng(5)
    a32 = handle(n, off, col)
    val = rng.standard_normal(len(col))
    val[::5] = 0.0  # stored zeros count as entries; values never matter
    a64 = handle(n, off, col, F64, val)
    for seed in cm.SEEDS:
        want = cm.expected(name, seed)
        assert_equals_model(a32.color(seed), want, (name, seed, "f32"))
        assert_equals_model(a64.color(seed), want, (name, seed, "f64"))
    assert_equals_model(a32.color(), cm.expected(name, 0), (name, "default seed"))


def test_empty(gpu):
    for dtype in (F32, F64):
        a = sm.SparseMatCRS.from_raw_parts(0, 0, [0], [], np.zeros(0, dtype))
        perm, stats = a.color(seed=1)
        assert len(perm) == 0 and len(stats["colors"]) == 0 and len(stats["color_counts"]) == 0
        assert (stats["n_colors"], stats["n_rounds"]) == (0, 0)
        n_colors, n_rounds = C.c_size_t(7), C.c_size_t(7)
        assert sm.lib().smh_crs_color(a._h, 0, None, None, C.byref(n_colors), C.byref(n_rounds)) == _lib.SMH_OK
        assert (n_colors.value, n_rounds.value) == (0, 0)


def test_what_the_tiny_cases_come_to(gpu):
    """on the device, without the model: isolated vertices take one colour in one round, a stored diagonal is no neighbour, the
    star's hub goes first"""
    for name in ("single", "single_with_diagonal", "diagonal_only", "isolated_5"):
        n, off, col = cm.case(name)
        perm, stats = handle(n, off, col).color()
        assert perm.tolist() == list(range(n)) and not stats["colors"].any()
        assert (stats["n_colors"], stats["n_rounds"]) == (1, 1) and stats["color_counts"].tolist() == [n]
    n, off, col = cm.case("star_5000")
    perm, stats = handle(n, off, col).color()
    assert stats["colors"][0] == 0 and (stats["colors"][1:] == 1).all() and (stats["n_colors"], stats["n_rounds"]) == (2, 2)
    n, off, col = cm.case("path_5")
    perm, stats = handle(n, off, col).color()
    assert perm.tolist() == [0, 2, 4, 1, 3] and stats["colors"].tolist() == [0, 1, 0, 1, 0] and stats["n_rounds"] == 3


def test_null_outputs_and_the_dev_form(gpu):
    name, seed = "grid_24x17_renumbered", 1
    n, off, col = cm.case(name)
    want = cm.expected(name, seed)
    a = handle(n, off, col)
    L = sm.lib()
    colors, perm = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    n_colors, n_rounds = C.c_size_t(), C.c_size_t()
    _lib.check(L.smh_crs_color(a._h, seed, colors.ctypes.data, None, C.byref(n_colors), None))
    assert np.array_equal(colors, want["colors"]) and n_colors.value == want["n_colors"]
    _lib.check(L.smh_crs_color(a._h, seed, None, perm.ctypes.data, None, C.byref(n_rounds)))
    assert np.array_equal(perm, want["perm"]) and n_rounds.value == want["n_rounds"]
    _lib.check(L.smh_crs_color(a._h, seed, None, None, None, None))
    # device arrays (n u32 in the storage of an f32 vector)
    dc, dp = sm.DenseVec.zeros(n, F32), sm.DenseVec.zeros(n, F32)
    n_colors, n_rounds = C.c_size_t(), C.c_size_t()
    _lib.check(L.smh_crs_color_dev(a._h, seed, C.c_void_p(dc.data_ptr()), C.c_void_p(dp.data_ptr()), C.byref(n_colors), C.byref(n_rounds)))
    assert np.array_equal(dc.to_numpy().view(np.uint32), want["colors"]) and np.array_equal(dp.to_numpy().view(np.uint32), want["perm"])
    assert (n_colors.value, n_rounds.value) == (want["n_colors"], want["n_rounds"])
    dp2 = sm.DenseVec.zeros(n, F32)
    _lib.check(L.smh_crs_color_dev(a._h, seed, None, C.c_void_p(dp2.data_ptr()), None, None))
    assert np.array_equal(dp2.to_numpy().view(np.uint32), want["perm"])
    dc2 = sm.DenseVec.zeros(n, F32)
    _lib.check(L.smh_crs_color_dev(a._h, seed, C.c_void_p(dc2.data_ptr()), None, None, None))
    assert np.array_equal(dc2.to_numpy().view(np.uint32), want["colors"])
    # the permutation on the device goes straight into permute_symmetric_dev
    h = C.c_void_p()
    _lib.check(L.smh_crs_permute_symmetric_dev(a._h, C.c_void_p(dp.data_ptr()), n, C.byref(h)))
    b = sm.SparseMatCRS(h, F32)
    assert np.array_equal(b.trisolve_levels("lower")["level_of_row"], want["colors"][want["perm"]])


def test_statuses(gpu):
    L = sm.lib()

    def status_of(call):
        with pytest.raises(_lib.SparseMatPanic) as e:
            call()
        return e.value.status

    assert L.smh_crs_color(None, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_color_dev(None, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
    rect = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [2, 0], np.ones(2, F32))
    assert status_of(rect.color) == _lib.SMH_ERR_NOT_SQUARE
    bad = sm.SparseMatCRS.from_raw_parts(3, 3, [0, 1, 2, 3], [0, 5, 1], np.ones(3, F32), validate=False)
    assert status_of(bad.color) == _lib.SMH_ERR_INDEX_RANGE
    # not square comes before the column check, as in rcm
    both = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [9, 0], np.ones(2, F32), validate=False)
    assert status_of(both.color) == status_of(both.rcm) == _lib.SMH_ERR_NOT_SQUARE
    # (SMH_ERR_CAPACITY needs a handle of 2^31 stored entries: the check is the one line of the set-up both orderings share)
    # the good handle still colours afterwards
    n, off, col = cm.case("path_5")
    assert handle(n, off, col).color()[0].tolist() == [0, 2, 4, 1, 3]


# ---- end to end on the device: what the ordering is for ---------------------------------------------------------------
def _grid_system(name, dtype):
    """the grid's pattern with values that round: off-diagonals in (-1, -0.5), a dominant diagonal"""
    n, off, col = cm.case(name)
    rng = np.random.default_rng(17)
    rows = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    val = -rng.uniform(0.5, 1.0, len(col))
    val[rows == col] = 2.0 * (3 if name.count("x") == 2 else 2) + rng.uniform(0.0, 1.0, n)
    return n, off, col, val.astype(dtype), rng.uniform(-1.0, 1.0, n).astype(dtype)


@pytest.mark.parametrize("name", sorted(cm.GRIDS))
def test_levels_and_solves_of_the_coloured_grid(gpu, name):
    dtype = F64 if "renumbered" in name else F32
    n, off, col, val, b = _grid_system(name, dtype)
    a = handle(n, off, col, dtype, val)
    perm, stats = a.color()
    assert_equals_model((perm, stats), cm.expected(name, 0), name)
    colors, n_colors = stats["colors"], stats["n_colors"]
    natural = a.trisolve_levels("lower")["n_levels"]
    B = a.permute_symmetric(perm)
    bo, bc, bv = rm.permute_symmetric(n, off, col, val, perm)
    go, gc, gv = B.raw_parts()
    assert np.array_equal(go, bo) and np.array_equal(gc, bc) and same(gv, bv)
    lower, upper = B.trisolve_levels("lower"), B.trisolve_levels("upper")
    assert np.array_equal(lower["level_of_row"], colors[perm]) and lower["n_levels"] == n_colors
    assert upper["n_levels"] <= n_colors
    assert lower["n_launches"] <= n_colors and upper["n_launches"] <= n_colors
    assert 4 <= n_colors <= 7 and (natural > 5 * n_colors or "renumbered" in name)
    bp = b[perm]
    for uplo in (tm.LOWER, tm.UPPER):
        plan = tm.Plan(bo, bc, uplo)
        assert plan.n_levels == (lower if uplo == tm.LOWER else upper)["n_levels"]
        for unit in (False, True):
            want = tm.trisolve(bo, bc, bv, bp, uplo, unit, plan=plan)
            got = B.trisolve(bp, uplo, unit)
            assert same(got, want), (name, uplo, unit, np.flatnonzero(got != want)[:5])


def test_sgs_pcg_on_the_coloured_system(gpu):
    """Row 2 of tests/sgs_model.py's table (the 40 x 33 grid, f64, tol 1e-10) in the natural ordering, coloured on the device and
    solved on the permuted matrix: x, the body count and r.r bit for bit the model's fed the device's product, as
    tests/test_sgs_gpu.py does it; the solution permuted back meets that file's residual bound -- sqrt(r.r) < tol -- on the
    ORIGINAL system, the residual recomputed in f64 from the stored values."""
    off, col, val, b, tol = sg.table_case(2, "natural")
    n = len(b)
    a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    perm, stats = a.color()
    assert_equals_model((perm, stats), cm.jones_plassmann(n, off, col, 0), "table row 2")
    B = a.permute_symmetric(perm)
    bo, bc, bv = rm.permute_symmetric(n, off, col, val, perm)
    assert B.trisolve_levels("lower")["n_levels"] == stats["n_colors"] < a.trisolve_levels("lower")["n_levels"] == 40 + 33 - 1
    bd = sm.DenseVec.from_vec(b)
    bp = bd.permute(perm)
    assert same(bp.to_numpy(), b[perm])
    x0 = np.zeros(n, val.dtype)
    for variant in ("stream", "auto"):
        B.prepare(variant)
        product = device_product(B, variant, bo, bc, bv)
        want = sg.sgs_pcg(bo, bc, bv, b[perm], x0, tol, 500, fused=is_fused(B, variant), product=product)
        assert 10 < want.iterations < 120 and math.sqrt(want.r_norm_squared) < tol
        solver = sm.SGSConjugateGradient(tol, 500, variant=variant)
        xp = sm.DenseVec.from_vec(x0)
        solver.solve(B, bp, xp)
        assert solver.iterations == want.iterations
        assert same(np.float64(solver.r_norm_squared), np.float64(want.r_norm_squared))
        assert same(xp.to_numpy(), want.x)
        x = xp.permute(perm, inverse=True).to_numpy()
        assert same(x[perm], want.x)
        A = np.zeros((n, n))
        np.add.at(A, (np.repeat(np.arange(n), np.diff(off.astype(np.int64))), col.astype(np.int64)), val.astype(np.float64))
        res = float(np.linalg.norm(b.astype(np.float64) - A @ x.astype(np.float64)))
        print("variant", variant, "bodies", solver.iterations, "recurrence residual", math.sqrt(solver.r_norm_squared), "true residual", res, "tol", tol)
        assert res < tol
