"""CPU: tests/bicgstab_model.py -- the contract of the device-resident BiCGSTAB (bicgstab.hip) -- on cases whose result is
known exactly (every breakdown code, the half-step stop, iter_max = 0: small integers, so every sum is exact in any order
and all three modes must give the same literals), its convergence on non-symmetric convection-diffusion systems in all
three summation modes, and the binding's declaration of the two entry points."""
import os
import re

import numpy as np
import pytest

import bicgstab_model as bm
import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
MODES = ["sequential", "device", "wide"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cases(dtype, mode):
    for name, a, b, iters, x, rr, breakdown, converged in bm.EXACT:
        off, col, val = bm.dense_to_crs(a, dtype)
        n = len(b)
        got = bm.bicgstab(off, col, val, np.array(b, dtype), np.zeros(n, dtype), 1e-6, 10, mode)
        assert got.iterations == iters, name
        assert got.x.dtype == dtype and got.x.tolist() == x, (name, got.x)
        assert got.r_norm_squared == rr, (name, got.r_norm_squared)
        assert got.breakdown == breakdown and got.converged is converged, name
        assert got.half_step is (name == "half-step stop"), name


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_iter_max_zero_enters_no_body(dtype, mode):
    """x = x0; r.r is the initial residual's: b - A x0 = (5, 4) - (4, 3) = (1, 1)."""
    off, col, val = bm.dense_to_crs([[2, 1], [0, 3]], dtype)
    x0 = np.array([1.5, 1.0], dtype)
    got = bm.bicgstab(off, col, val, np.array([5, 4], dtype), x0, 1e-6, 0, mode)
    assert got.iterations == 0 and got.x.tolist() == [1.5, 1.0] and got.r_norm_squared == 2.0
    assert got.breakdown == 0 and got.converged is False


GRIDS = [(5, .5), (12, .5), (16, 1.0), (23, .25)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_converges_on_convection_diffusion(dtype):
    """Every mode converges without a breakdown in fewer than 200 bodies, to max|x - x*| <= 1e-8 (f64, tol 1e-10) /
    1e-3 (f32, tol 1e-4): the issue's bounds.  With this file's x* (seeded by g) and sequential sums the cases take 16 to 66
    bodies in f64 and 11 to 40 in f32 and end at most 5.5e-11 / 1.0e-4 away from x* (the figures are printed), so the bounds
    leave the other summation orders a factor of 180 in f64 and of ten in f32.  Both kinds of stop occur in "device" mode."""
    tol, bound = (1e-10, 1e-8) if dtype == np.float64 else (1e-4, 1e-3)
    half_steps = []
    for g, c in GRIDS:
        off, col, val, b, x_star = bm.convdiff_system(g, c, dtype)
        for mode in MODES:
            got = bm.bicgstab(off, col, val, b, np.zeros(g * g, dtype), tol, 200, mode)
            err = float(np.abs(got.x - x_star).max())
            print(np.dtype(dtype).name, g, c, mode, got.iterations, got.half_step, err)
            assert got.converged and got.breakdown == 0 and got.iterations < 200, (g, c, mode, got.iterations, got.breakdown)
            assert np.sqrt(got.r_norm_squared) < tol
            assert err <= bound, (g, c, mode, err)
            if mode == "device":
                half_steps.append(got.half_step)
    assert any(half_steps) and not all(half_steps), half_steps


def test_generators():
    off, col, val = bm.convdiff2d(3, .5, np.float64)
    assert off.tolist() == [0, 3, 7, 10, 14, 19, 23, 26, 30, 33]
    assert col[off[4]:off[5]].tolist() == [4, 3, 5, 1, 7] and val[off[4]:off[5]].tolist() == [4.5, -1.5, -1.0, -1.25, -0.75]
    assert col[off[0]:off[1]].tolist() == [0, 1, 3] and val[off[0]:off[1]].tolist() == [4.5, -1.0, -0.75]
    off, col, val = bm.tridiag_ns(4, .5, np.float32, seed=1)
    assert off.tolist() == [0, 2, 5, 8, 10] and col.tolist() == [0, 1, 0, 1, 2, 1, 2, 3, 2, 3]
    assert val[[2, 5, 8]].tolist() == [-1.5] * 3 and val[[1, 4, 7]].tolist() == [-1.0] * 3
    assert ((val[[0, 3, 6, 9]] >= 2.5) & (val[[0, 3, 6, 9]] < 3.5)).all()
    for n in (0, 1):
        off, col, val = bm.tridiag_ns(n, .5, np.float64)
        assert off.tolist() == [0, 1][:n + 1] and len(col) == len(val) == n


def test_binding_and_header_declare_both_entry_points():
    header = open(os.path.join(ROOT, "include", "sparsemat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    # (the host entry takes 11 arguments, the DenseVec one 10: two lengths less, check_every more)
    for name, n_args in (("smh_bicgstab_solve", 11), ("smh_bicgstab_solve_vec", 10)):
        assert name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == n_args, (name, len(argtypes))
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    # the statuses are decided before any device call: a NULL handle is refused where there is no device either
    L = sm.lib()
    assert L.smh_bicgstab_solve(None, None, 0, None, 0, 1e-10, 5, 0, None, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_bicgstab_solve_vec(None, None, None, 1e-10, 5, 0, 0, None, None, None) == _lib.SMH_ERR_INVALID
    assert b"NULL handle" in L.smh_last_error()


class CountedProduct:
    """oracle.spmv as a ``product`` callable that counts its calls; bump = (c, k): in the c-th call the element of k-th largest
    magnitude moves by one ulp."""

    def __init__(self, off, col, val, bump=(None, 0)):
        self.parts, self.bump, self.calls = (off, col, val), bump, 0

    def __call__(self, v):
        y = oracle.spmv(*self.parts, v)
        if self.calls == self.bump[0]:
            j = int(np.argsort(-np.abs(y), kind="stable")[self.bump[1]])
            y[j] = np.nextafter(y[j], y.dtype.type(np.inf))
        self.calls += 1
        return y


def results(r):
    return r.x.tobytes(), r.iterations, r.rr.tobytes(), r.breakdown, r.converged, r.half_step, np.array(r.ss_list).tobytes(), np.array(r.rr_list).tobytes(), r.r.tobytes(), r.p.tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_product_callable_is_what_the_model_consumes(dtype, mode):
    """product = the oracle's own product: the default's bytes (x, the last r.r, every s.s and r.r, the body count, the breakdown
    code), 1 + 2 * bodies calls (the initial residual's, A p and A s of every body), one less after a half-step stop, and
    the exact cases' breakdowns.  One ulp on one element of ANY single call changes the result (x, r, p, an s.s or an r.r: one
    ulp on one element seldom moves a dot, so the last call's shows in r and p alone): no product comes from anywhere else.
    (It can also round away in v * alpha, so for each call the elements are tried in order of magnitude, at most eight of
    them, until one shows.)"""
    off, col, val, b, _ = bm.convdiff_system(12, 0.5, dtype)
    x0 = np.random.default_rng(3).uniform(-1, 1, 144).astype(dtype)
    bodies = 5
    want = bm.bicgstab(off, col, val, b, x0, 0.0, bodies, mode)
    assert want.iterations == bodies and want.breakdown == 0
    counted = CountedProduct(off, col, val)
    assert results(bm.bicgstab(off, col, val, b, x0, 0.0, bodies, mode, product=counted)) == results(want)
    assert counted.calls == 1 + 2 * bodies
    for call in range(1 + 2 * bodies):
        for k in range(8):
            bumped = bm.bicgstab(off, col, val, b, x0, 0.0, bodies, mode, product=CountedProduct(off, col, val, bump=(call, k)))
            if results(bumped) != results(want):
                break
        else:
            raise AssertionError("call %d of the product is not consumed" % call)
    # a stop at the half step of body 3 (s.s_3 under tol, everything before it above) and one at its full step
    norms = np.sqrt(np.array([[float(s), float(r)] for s, r in zip(want.ss_list, want.rr_list)])).reshape(-1)
    for event, half in ((4, True), (5, False)):
        lo, hi = norms[event], norms[:event].min()
        if not lo < hi:
            continue
        tol = 0.5 * (lo + hi)
        stopped = bm.bicgstab(off, col, val, b, x0, tol, bodies, mode)
        assert stopped.iterations == 3 and stopped.converged and stopped.half_step is half
        counted = CountedProduct(off, col, val)
        assert results(bm.bicgstab(off, col, val, b, x0, tol, bodies, mode, product=counted)) == results(stopped)
        assert counted.calls == 1 + 2 * 3 - (1 if half else 0)
    for name, a, b, iters, x, rr, breakdown, converged in bm.EXACT:
        off, col, val = bm.dense_to_crs(a, dtype)
        counted = CountedProduct(off, col, val)
        got = bm.bicgstab(off, col, val, np.array(b, dtype), np.zeros(len(b), dtype), 1e-6, 10, mode, product=counted)
        assert (got.iterations, got.x.tolist(), got.r_norm_squared, got.breakdown, got.converged) == (iters, x, rr, breakdown, converged), name
        assert counted.calls == 1 + 2 * iters - (1 if breakdown == 2 or name == "half-step stop" else 0), name
