"""CPU: tests/refine_model.py, the numpy restatement of the mixed-precision refinement (smh_refine_solve*), and the conversion rule
of smh_crs_cast / smh_vec_cast.

* the scale e = floor(ilogb(rr) / 2) on hand cases;
* tol already met: no outer step and no inner call;
* on three SPD grids and on convdiff2d(24, 1.0) the f32 model alone stops with a true residual far above tol, the refinement's true
  residual (numpy, f64) is below 2 tol, and its inner bodies stay within the measured ratio + 1/4 of the f64 model's bodies;
* every case of tests/refine_cases.py -- the GPU file's -- moves a bit or a count under each wrong variant listed for it;
* the conversion's rounding on hand cases; the declarations exist and refuse bad arguments without a device."""
import ctypes as C
import math

import numpy as np
import pytest

import bicgstab_model as bm
import cg_model
import gmres_model as gm
import oracle
import refine_cases as rc
import refine_model as rm
import sgs_model
import sparsemat_amd as sm
from kernel_forms import same
from sparsemat_amd import _lib

F32, F64 = np.float32, np.float64


# ---- the scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rr, e", [(1.0, 0), (3.99, 0), (4.0, 1), (2.0 ** -61, -31), (5e-324, -537), (2.0 ** -1070, -535), (2.0 ** 1000, 500),
                                   (2.0, 0), (0.5, -1), (0.25, -1), (0.24, -2)])
def test_scale_on_hand_cases(rr, e):
    """e from math.frexp; (r 2^-e)^2 = rr 2^(-2e) lies in [1, 4) -- exactly, the scaling is by a power of two"""
    assert rm.scale_exponent(rr) == e
    m, ex = math.frexp(rr)
    assert rm.scale_exponent(rr) == (ex - 1) // 2
    scaled = math.ldexp(rr, -2 * e)
    assert 1.0 <= scaled < 4.0 and math.frexp(scaled)[0] == m
    assert rm.scale_exponent(rr, up=True) == e + ((ex - 1) % 2)  # (the wrong variant differs on odd exponents alone)


def test_scale_of_a_non_finite_rr_is_zero():
    assert rm.scale_exponent(float("nan")) == rm.scale_exponent(float("inf")) == 0


def test_tol_already_met_takes_no_step():
    off, col, val, b, x0 = rc.tridiag(50)

    def inner(r, d):
        raise AssertionError("the inner solve was called")
    res = rm.refine(lambda v: oracle.spmv(off, col, val, v), inner, b, x0, 1e3)
    assert (res.outer, res.iterations, res.code) == (0, 0, 0) and same(res.x, x0)
    assert same(res.rr, cg_model.device_sum(b * b, cg_model.pcg_grid(50), 2, from_first=True))


# ---- accuracy and cost against the f64 models ------------------------------------------------------------------------------------------
# (grid, measured inner bodies / f64 bodies with inner_tol = 1e-4 and tol = 1e-10 |b|): DESIGN.md section 4, "Mixed-precision refinement"
GRIDS = [((24, 17, 1.0, 1), 1.567), ((40, 33, 1.0, 2), 1.362), ((32, 32, 2.0, 3), 1.390)]


def true_residual(off, col, val, b, x):
    return float(np.linalg.norm(b - oracle.spmv(off, col, val, np.asarray(x, F64))))


@pytest.mark.parametrize("grid, ratio", GRIDS, ids=["24x17", "40x33", "32x32"])
def test_refinement_reaches_tol_on_spd_grids_where_f32_stalls(grid, ratio):
    nx, ny, spread, seed = grid
    off, col, val = sgs_model.lap2d(nx, ny, F64, seed, spread)
    n = nx * ny
    b = np.random.default_rng(50 + seed).uniform(-1, 1, n)
    tol = 1e-10 * float(np.linalg.norm(b))
    val32 = rm.cast(val, F32)
    alone = cg_model.cg(off, col, val32, b.astype(F32), np.zeros(n, F32), tol, 3000)
    assert true_residual(off, col, val, b, alone.x) > 100 * tol
    wide = cg_model.cg(off, col, val, b, np.zeros(n), tol, 5000)
    res = rm.refine(lambda v: oracle.spmv(off, col, val, v), rm.inner_cg(off, col, val32), b, np.zeros(n), tol)
    print("bodies: f64 %d, refinement %d in %d outer steps, ratio %.3f" % (wide.iterations, res.iterations, res.outer, res.iterations / wide.iterations))
    assert res.code == 0 and 2 <= res.outer <= 4
    assert true_residual(off, col, val, b, res.x) < 2 * tol
    assert res.iterations <= (ratio + 0.25) * wide.iterations


@pytest.mark.parametrize("solver, ratio", [("bicgstab", 1.574), ("gmres", 1.096)])
def test_refinement_reaches_tol_on_convdiff(solver, ratio):
    off, col, val = bm.convdiff2d(24, 1.0, F64)
    n = 576
    b = np.random.default_rng(77).uniform(-1, 1, n)
    tol = 1e-10 * float(np.linalg.norm(b))
    val32 = rm.cast(val, F32)
    if solver == "bicgstab":
        alone = bm.bicgstab(off, col, val32, b.astype(F32), np.zeros(n, F32), tol, 500)
        wide = bm.bicgstab(off, col, val, b, np.zeros(n), tol, 5000)
        inner = rm.inner_bicgstab(off, col, val32)
    else:
        alone = gm.gmres(off, col, val32, b.astype(F32), np.zeros(n, F32), tol, 500, 30)
        wide = gm.gmres(off, col, val, b, np.zeros(n), tol, 5000, 30)
        inner = rm.inner_gmres(off, col, val32, 30)
    assert true_residual(off, col, val, b, alone.x) > 100 * tol
    res = rm.refine(lambda v: oracle.spmv(off, col, val, v), inner, b, np.zeros(n), tol)
    print("bodies: f64 %d, refinement %d in %d outer steps, ratio %.3f" % (wide.iterations, res.iterations, res.outer, res.iterations / wide.iterations))
    assert res.code == 0 and wide.breakdown == 0
    assert true_residual(off, col, val, b, res.x) < 2 * tol
    assert res.iterations <= (ratio + 0.25) * wide.iterations


# ---- the GPU file's cases under the wrong variants -----------------------------------------------------------------------------------
def differs(got, want):
    return not (same(got.x, want.x) and got.outer == want.outer and got.iterations == want.iterations and same(F64(got.rr), F64(want.rr))
                and got.code == want.code)


@pytest.mark.parametrize("case", rc.CASES, ids=[c.name for c in rc.CASES])
def test_every_gpu_case_moves_under_each_wrong_variant_that_can_touch_it(case):
    system = case.system()
    want = rc.model(case, system=system)
    assert want.code == case.code
    for wrong in case.wrong:
        assert differs(rc.model(case, wrong, system=system), want), (case.name, wrong)
    off, col, val, b, x0 = system
    if case.code == 0 and case.tol < 1.0 and case.n:
        assert true_residual(off, col, val, b, want.x) < 2 * case.tol
    assert {w for c in rc.CASES for w in c.wrong} == set(rc.ALL_WRONG)  # (no wrong variant goes unseen)


def test_the_stops_of_the_cases():
    by = {name: rc.model(rc.BY_NAME[name]) for name in ("tol_met", "outer_max1", "stall", "zero_b", "nan_b")}
    assert (by["tol_met"].outer, by["tol_met"].iterations) == (0, 0)
    assert (by["outer_max1"].outer, by["outer_max1"].code) == (1, 1)
    stall = by["stall"]
    assert stall.code == 2 and stall.outer >= 3 and not (stall.rr_list[-1] < stall.rr) and same(F64(stall.rr), F64(stall.rr_list[-2]))
    assert (by["zero_b"].outer, by["zero_b"].code, float(by["zero_b"].rr)) == (0, 0, 0.0)
    nan = by["nan_b"]
    assert (nan.outer, nan.code) == (1, 2) and same(nan.x, rc.BY_NAME["nan_b"].system()[4]) and math.isnan(nan.rr)


# ---- the conversion --------------------------------------------------------------------------------------------------------------------
def test_conversion_rounds_to_nearest_even_on_hand_cases():
    big = float(np.finfo(F32).max)
    first_over = big + 2.0 ** 103  # the midpoint between the largest finite f32 and 2^128: ties to even go up
    cases = [(1.0 + 2.0 ** -24, 1.0), (1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -22), (big, big), (np.nextafter(first_over, 0.0), big), (first_over, np.inf),
             (-first_over, -np.inf), (2.0 ** -149, 2.0 ** -149), (2.0 ** -150, 0.0), (1.5 * 2.0 ** -149, 2.0 ** -148), (2.0 ** -130 * (1 + 2.0 ** -30), 2.0 ** -130),
             (-0.0, -0.0), (np.inf, np.inf)]
    src = np.array([c[0] for c in cases], F64)
    want = np.array([c[1] for c in cases], F32)
    got = rm.cast(src, F32)
    assert same(got, want), (got, want)
    assert np.signbit(got[10]) and rm.overflow_count(src) == 2
    assert np.isnan(rm.cast(np.array([np.nan]), F32))[0]
    back = rm.cast(got, F64)
    assert back.dtype == F64 and same(rm.cast(back, F32), got)  # (f32 -> f64 is exact)


# ---- the declarations ----------------------------------------------------------------------------------------------------------------
def test_declarations_exist_and_refuse_bad_arguments_before_any_device_call():
    L = sm.lib()
    for name in ("smh_crs_cast", "smh_vec_cast", "smh_refine_solve", "smh_refine_solve_vec"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    h, over = C.c_void_p(), C.c_size_t(7)
    assert L.smh_crs_cast(None, _lib.SMH_F32, C.byref(h), C.byref(over)) == _lib.SMH_ERR_INVALID
    assert L.smh_vec_cast(None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_refine_solve(None, None, 0, 0, None, None, None, 0, None, 0, 1e-9, 0, 0.0, 0, 0, 0, 0, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_refine_solve_vec(None, None, 0, 0, None, None, None, None, 1e-9, 0, 0.0, 0, 0, 0, 0, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert b"NULL" in L.smh_last_error()
    assert (_lib.SMH_INNER_CG, _lib.SMH_INNER_BICGSTAB, _lib.SMH_INNER_GMRES, _lib.SMH_PRECOND_FSAI) == (0, 1, 2, 4)
    with pytest.raises(ValueError):
        sm.IterativeRefinement(inner="sor")
    with pytest.raises(ValueError):
        sm.IterativeRefinement(precond="amg")
    s = sm.IterativeRefinement()
    assert (s.tol, s.outer_max, s.inner, s.precond, s.inner_tol, s.inner_iter_max, s.restart) == (1e-12, 20, "cg", None, 1e-4, 10_000, 30)
    assert hasattr(sm.SparseMatCRS, "astype") and hasattr(sm.DenseVec, "astype")
