"""CPU: tests/gmres_model.py -- the contract of the device-resident restarted GMRES (gmres.hip) -- on cases whose result is known
exactly, the minimisation property of one cycle against a dense f64 least-squares solve on the same Krylov space, the
skew-dominated systems on which BiCGSTAB stagnates or breaks down, the convection-diffusion grids of test_bicgstab_model.py,
the sensitivity of the GPU file's cases to every wrong variant of the arithmetic, the product callable, and the declaration of
the two entry points."""
import math
import os
import re

import numpy as np
import pytest

import bicgstab_model as bm
import gmres_cases
import gmres_model as gm
import sparsemat_amd as sm
from sparsemat_amd import _lib
from test_bicgstab_model import GRIDS, CountedProduct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
MODES = ["sequential", "device", "wide"]


def exact(a):
    return next(e for e in bm.EXACT if e[0] == a)


def true_residual(off, col, val, b, x):
    """||b - A x|| in f64 (longdouble sums)"""
    off = np.asarray(off, np.int64)
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    ax = np.zeros(len(b), np.longdouble)
    np.add.at(ax, rows, np.asarray(val, np.longdouble) * np.asarray(x, np.longdouble)[np.asarray(col, np.int64)])
    return float(np.sqrt(np.sum((np.asarray(b, np.longdouble) - ax) ** 2)))


# ---- exact cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cases(dtype, mode):
    """The two non-singular systems on which BiCGSTAB breaks down are solved in two bodies (n = 2: the second body exhausts the
    Krylov space).  v_0 = r / sqrt(5) is not exact, so x is held to 4 eps * max|x| of the literal (a handful of roundings of
    numbers of size one in the two bodies), and the codes to what the arithmetic allows: hn of the second body is a rounding
    error or zero, so the stop is the estimate's (code 0) or the exhausted space's (code 1)."""
    eps = np.finfo(dtype).eps
    for name, x_want in (("breakdown 1", [1.0, -0.5]), ("breakdown 2 (skew)", [0.0, 1.0])):
        _, a, b = exact(name)[:3]
        off, col, val = bm.dense_to_crs(a, dtype)
        got = gm.gmres(off, col, val, np.array(b, dtype), np.zeros(2, dtype), 1e-6, 10, 20, mode)
        assert got.iterations == 2 and got.cycles == 1 and got.breakdown in (0, 1), (name, got.iterations, got.breakdown)
        print(np.dtype(dtype).name, mode, name, got.x.tolist(), got.breakdown)
        assert got.x.dtype == dtype and np.abs(got.x - np.array(x_want)).max() <= 4 * eps, (name, got.x)
        assert math.sqrt(got.r_norm_squared) < 1e-6
    # the skew case is exact throughout: r = (1, 0), beta = 1, w = A v_0 = (0, -1), h = 0, hn = 1, c_0 = 0, s_0 = 1, g = (0, -1);
    # w = A (0, -1) = (-1, 0), h_0 = -1, h_1 = 0, hn = 0: breakdown 1; rotated h = (0, 1), R = [[1, 0], [0, 1]], y = (0, -1) ...
    _, a, b = exact("breakdown 2 (skew)")[:3]
    off, col, val = bm.dense_to_crs(a, dtype)
    got = gm.gmres(off, col, val, np.array(b, dtype), np.zeros(2, dtype), 1e-6, 10, 20, mode)
    assert got.x.tolist() == [0.0, 1.0] and got.breakdown == 1 and got.r_norm_squared == 0.0 and got.estimates == [1.0, 0.0]
    # A = 2 I, b = e_1: w = 2 e_1, h1 = 2, w = 0, hn = 0: breakdown 1 in one body (|g_1| = 0 < tol holds with it), x = e_1 / 2
    off, col, val = bm.dense_to_crs(2 * np.eye(5), dtype)
    b = np.zeros(5, dtype)
    b[0] = 1
    got = gm.gmres(off, col, val, b, np.zeros(5, dtype), 1e-6, 10, 20, mode)
    assert (got.iterations, got.cycles, got.breakdown, got.r_norm_squared) == (1, 1, 1, 0.0)
    assert got.x.tolist() == [0.5, 0, 0, 0, 0]
    # b = A x0: beta == 0, breakdown 2, no body -- whatever iter_max
    off, col, val = bm.dense_to_crs([[2, 1], [0, 3]], dtype)
    x0 = np.array([1.5, 1.0], dtype)
    for iter_max in (10, 0):
        got = gm.gmres(off, col, val, np.array([4, 3], dtype), x0, 1e-6, iter_max, 20, mode)
        assert (got.iterations, got.cycles, got.breakdown, got.r_norm_squared) == (0, 0, 2, 0.0) and got.x.tolist() == [1.5, 1.0]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_iter_max_zero_enters_no_body(dtype, mode):
    """x = x0; r.r is the initial residual's: b - A x0 = (5, 4) - (4, 3) = (1, 1); the first v_0 has been formed."""
    off, col, val = bm.dense_to_crs([[2, 1], [0, 3]], dtype)
    got = gm.gmres(off, col, val, np.array([5, 4], dtype), np.array([1.5, 1.0], dtype), 1e-6, 0, 20, mode)
    assert got.iterations == 0 and got.x.tolist() == [1.5, 1.0] and got.r_norm_squared == 2.0
    assert got.breakdown == 0 and got.cycles == 1


# ---- the minimisation property ------------------------------------------------------------------------------------------------
def dense_case(n, dtype, seed):
    """A = 2 I + E, |E_ik| < 0.5 / sqrt(n): ||E||_2 <= ||E||_F < 0.5 * sqrt(n), far less in fact; here cond(A) < 3 is asserted"""
    rng = np.random.default_rng(seed)
    a = (2 * np.eye(n) + rng.uniform(-0.5, 0.5, (n, n)) / math.sqrt(n)).astype(dtype)
    assert np.linalg.cond(a.astype(np.float64)) < 3
    return a, rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_cycle_minimises_the_residual_over_the_krylov_space(dtype):
    """One cycle of j bodies (restart = iter_max = j, tol = 0) on A = 2 I + E (n = 24, cond < 3) against the f64 least-squares
    minimiser over x0 + span(r0, A r0, .., A^(j-1) r0) (an orthonormal basis of it by QR in f64).

    The bound.  u = eps(T) / 2.  A sum of n products is off by at most n u sum|terms| (sequential sums, the deepest of the three
    modes), a row of A likewise.  A body makes 2 (j + 1) dots and as many updates of w, the cycle end 2 j + 1 updates of x and r:
    every entry of every vector is the end of a chain of at most D = n + 4 (j + 1) + 8 rounded operations on numbers of size
    ||A|| ||r0|| at most (the basis has norm one, |h| <= ||A||, |y| <= ||r0|| / sigma_min; here ||A|| < 3, kappa < 3), and the j
    bodies add up: the true residual, the estimate |g_j| and sqrt(rr) each lie within  B = 4 j D u ||r0||  of the least-squares
    minimum (4: ||A|| and the two-norm of a vector of such errors against its largest entry, generously).  The orthogonality
    max|V^T V - I| is measured on the sequential model and asserted there at (j + 1) D u (Gram-Schmidt twice: O(u) times the depth
    of the dots, per column); the other modes get TWICE that figure (their sums are no deeper)."""
    n = 24
    u = np.finfo(dtype).eps / 2
    a, b, x0 = dense_case(n, dtype, 7)
    off, col, val = bm.dense_to_crs(a, dtype)
    a64, b64, x64 = a.astype(np.float64), b.astype(np.float64), x0.astype(np.float64)
    r0 = b64 - a64 @ x64
    for j in (1, 2, 5, 9):
        k = np.stack([np.linalg.matrix_power(a64, p) @ r0 for p in range(j)], axis=1)
        q, _ = np.linalg.qr(k)
        coef, *_ = np.linalg.lstsq(a64 @ q, r0, rcond=None)
        best = float(np.linalg.norm(r0 - a64 @ (q @ coef)))
        depth = n + 4 * (j + 1) + 8
        bound = 4 * j * depth * u * float(np.linalg.norm(r0))
        ortho_bound = (j + 1) * depth * u
        for mode in MODES:
            got = gm.gmres(off, col, val, b, x0, 0.0, j, j, mode)
            assert got.iterations == j and got.cycles == 1 and got.breakdown == 0
            true = true_residual(off, col, val, b, got.x)
            print(np.dtype(dtype).name, j, mode, best, true - best, got.estimates[-1] - best, math.sqrt(got.r_norm_squared) - best, bound)
            assert abs(true - best) <= bound, (j, mode, true, best, bound)
            assert abs(got.estimates[-1] - best) <= bound, (j, mode, got.estimates[-1], best)
            assert abs(math.sqrt(got.r_norm_squared) - best) <= bound, (j, mode, got.r_norm_squared, best)
            v = np.stack(got.basis, axis=1).astype(np.float64)
            ortho = float(np.abs(v.T @ v - np.eye(j + 1)).max())
            print("   max|VtV - I|", ortho, ortho_bound)
            assert ortho <= (1 if mode == "sequential" else 2) * ortho_bound, (j, mode, ortho)


# ---- the skew-dominated systems ---------------------------------------------------------------------------------------------------
SKEW = [(40, 0.25), (100, 0.125)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_skew_dominated_systems(dtype):
    """tridiag(-1, delta, +1): GMRES(20) and GMRES(n) converge in every mode within 1000 bodies and the TRUE residual of their x is
    below 2 tol (the estimate |g_j| < tol stopped the loop; the rebuilt residual and the estimate agree to rounding);
    bicgstab_model at n = 100 does not converge within 400 bodies or breaks down."""
    tol = 1e-10 if dtype == np.float64 else 1e-4
    for n, delta in SKEW:
        off, col, val, b, x_star = gm.skew_system(n, delta, dtype)
        x0 = np.zeros(n, dtype)
        for restart in (20, n):
            for mode in MODES:
                got = gm.gmres(off, col, val, b, x0, tol, 1000, restart, mode)
                true = true_residual(off, col, val, b, got.x)
                print(np.dtype(dtype).name, n, restart, mode, got.iterations, got.cycles, got.breakdown, true / tol)
                assert got.iterations < 1000 and got.estimates[-1] < tol and got.breakdown in (0, 1), (n, restart, mode, got.iterations)
                assert true <= 2 * tol, (n, restart, mode, true)
                if restart == n:
                    assert got.iterations <= n and got.cycles == 1
        if n == 100:
            for mode in MODES:
                bi = bm.bicgstab(off, col, val, b, x0, tol, 400, mode)
                print("   bicgstab", mode, bi.iterations, bi.breakdown, bi.converged)
                assert not bi.converged and (bi.breakdown != 0 or bi.iterations == 400), (mode, bi.iterations, bi.breakdown)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_converges_on_convection_diffusion(dtype):
    """The grids and the bounds of test_bicgstab_model.py (max|x - x*| <= 1e-8 at tol 1e-10 in f64, 1e-3 at tol 1e-4 in f32):
    GMRES(30) and GMRES(5) converge in every mode."""
    tol, bound = (1e-10, 1e-8) if dtype == np.float64 else (1e-4, 1e-3)
    for g, c in GRIDS:
        off, col, val, b, x_star = bm.convdiff_system(g, c, dtype)
        for restart in (30, 5):
            for mode in MODES:
                got = gm.gmres(off, col, val, b, np.zeros(g * g, dtype), tol, 2000, restart, mode)
                err = float(np.abs(got.x - x_star).max())
                print(np.dtype(dtype).name, g, c, restart, mode, got.iterations, got.cycles, err)
                assert got.iterations < 2000 and got.breakdown == 0 and got.estimates[-1] < tol, (g, c, restart, mode, got.iterations)
                assert err <= bound, (g, c, restart, mode, err)


# ---- what the bit comparisons of the GPU file can tell apart ----------------------------------------------------------------------
def bits(r):
    return r.x.tobytes(), r.iterations, r.cycles, r.rr.tobytes(), r.breakdown


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_cases_move_under_every_wrong_variant(dtype):
    """Every case tests/test_gmres_gpu.py compares bit for bit (gmres_cases.BIT_CASES; the large size runs the same arithmetic) gives
    other bits under each wrong variant it can tell apart: an FMA in the update, one Gram-Schmidt pass, the update over c
    descending, modified Gram-Schmidt, sequential sums.  What cannot tell: the exact cases and the all-NaN one (case.exact), a
    solve without a body, the sizes n <= 5 (sums of a handful of terms and a Krylov space exhausted after n bodies: they are there
    for the kernels' edge paths), and restart 1 for the orders over c and the FMA (one column, and w reaches the result through
    hn alone).  Everything else must move."""
    for case in gmres_cases.BIT_CASES:
        off, col, val, b, x0 = case.system(dtype)
        want = gm.gmres(off, col, val, b, x0, case.tol(dtype), case.iter_max, case.restart)
        for wrong in ("fma", "one pass", "descending", "mgs", "sequential"):
            if wrong == "sequential":
                other = gm.gmres(off, col, val, b, x0, case.tol(dtype), case.iter_max, case.restart, mode="sequential")
            else:
                other = gm.gmres(off, col, val, b, x0, case.tol(dtype), case.iter_max, case.restart, wrong=wrong)
            blind = case.exact or case.n <= 5 or want.iterations == 0 or (case.restart == 1 and wrong in ("fma", "descending", "mgs"))
            if not blind:
                assert bits(other) != bits(want), (case.name, wrong)


# ---- the product callable -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_product_callable_is_what_the_model_consumes(dtype, mode):
    """product = the oracle's own product: the default's bytes with 1 + bodies calls (the initial residual's and one per body: none
    at a cycle end), and one ulp on one element of ANY single call changes the result (for each call the elements are tried in
    order of magnitude, at most eight of them, until one shows)."""
    off, col, val, b, _ = bm.convdiff_system(12, 0.5, dtype)
    x0 = np.random.default_rng(3).uniform(-1, 1, 144).astype(dtype)
    bodies, restart = 7, 3  # two restarts and a cycle cut short by iter_max
    want = gm.gmres(off, col, val, b, x0, 0.0, bodies, restart, mode)
    assert want.iterations == bodies and want.cycles == 3 and want.breakdown == 0
    counted = CountedProduct(off, col, val)
    assert bits(gm.gmres(off, col, val, b, x0, 0.0, bodies, restart, mode, product=counted)) == bits(want)
    assert counted.calls == 1 + bodies
    for call in range(1 + bodies):
        for k in range(8):
            bumped = gm.gmres(off, col, val, b, x0, 0.0, bodies, restart, mode, product=CountedProduct(off, col, val, bump=(call, k)))
            if bits(bumped) != bits(want) or any(not np.array_equal(p, q) for p, q in zip(bumped.basis, want.basis)):
                break
        else:
            raise AssertionError("call %d of the product is not consumed" % call)


def test_generator():
    off, col, val = gm.tridiag_skew(4, 0.25, np.float32)
    assert off.tolist() == [0, 2, 5, 8, 10] and col.tolist() == [0, 1, 0, 1, 2, 1, 2, 3, 2, 3]
    assert val.tolist() == [0.25, 1, -1, 0.25, 1, -1, 0.25, 1, -1, 0.25]
    off, col, val, b, x_star = gm.skew_system(5, 0.125, np.float64)
    assert x_star.tolist() == [-3, -2, -1, 0, 1] and b.tolist() == [-2.375, 1.75, 1.875, 2.0, 0.125]


def test_binding_and_header_declare_both_entry_points():
    header = open(os.path.join(ROOT, "include", "sparsemat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    # (the host entry takes 13 arguments, the DenseVec one 12: two lengths less, check_every more)
    for name, n_args in (("smh_gmres_solve", 13), ("smh_gmres_solve_vec", 12)):
        assert name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == n_args, (name, len(argtypes))
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    # the statuses are decided before any device call: a NULL handle is refused where there is no device either
    L = sm.lib()
    assert L.smh_gmres_solve(None, None, 0, None, 0, 1e-10, 5, 30, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert b"NULL handle" in L.smh_last_error()
    assert L.smh_gmres_solve_vec(None, None, None, 1e-10, 5, 30, 0, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert b"NULL handle" in L.smh_last_error()
    assert sm.GMRES(1e-8, 50).restart == 30 and sm.GMRES(1e-8, 50, restart=7).cycles is None
