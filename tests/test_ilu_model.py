"""CPU: tests/ilu_model.py -- the numpy restatement of ILU(0) and of its application.  A case worked out by hand, the dense
pattern against a plain Doolittle LU, the componentwise residual bound on the pattern, every matrix of the GPU file moving a bit
under each wrong variant it can tell apart, the body counts that are the reason the preconditioner exists, and the new entry
points' table entries and argument statuses (which need no device)."""
import ctypes as C

import numpy as np
import pytest

import ilu_cases as ic
import ilu_model as im
import sgs_model as sg
import sparsemat_amd as sm
import trisolve_model as tm
from sparsemat_amd import _lib

F32, F64 = np.float32, np.float64
DTYPES = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_worked_by_hand(dtype):
    """A = [2 1 . 1; 4 3 1 .; . 2 4 1; 2 . 2 5], every value exact:
    row 1: l10 = 4/2 = 2; (1,1) = 3 - 2*1 = 1; the fill at (1,3) is dropped                         -> 2 1 1
    row 2: l21 = 2/1 = 2; (2,2) = 4 - 2*1 = 2                                                      -> 2 2 1
    row 3: l30 = 2/2 = 1; (3,3) = 5 - 1*1 = 4 ((3,1) dropped); l32 = 2/2 = 1; (3,3) = 4 - 1*1 = 3  -> 1 1 3"""
    off, col, val = tm.from_rows([[(0, 2), (1, 1), (3, 1)], [(0, 4), (1, 3), (2, 1)], [(1, 2), (2, 4), (3, 1)], [(0, 2), (2, 2), (3, 5)]], dtype)
    for vector in (False, True):
        w, zp, d = im.ilu0(off, col, val, vector=vector, counts=True)
        assert w.dtype == dtype and w.tolist() == [2, 1, 1, 2, 1, 1, 2, 2, 1, 1, 1, 3] and zp is None
        assert d.tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 2]
    L, U = im.dense_factors(off, col, w)
    assert L.tolist() == [[1, 0, 0, 0], [2, 1, 0, 0], [0, 2, 1, 0], [1, 0, 1, 1]] and U.tolist() == [[2, 1, 0, 1], [0, 1, 1, 0], [0, 0, 2, 1], [0, 0, 0, 3]]
    # z = U^-1 L^-1 r:  L w = r = (2, 5, 5, 8) gives w = (2, 1, 3, 3);  U z = w gives z = (0, 0, 1, 1)... checked as L U z = r
    z = im.ilu_apply(off, col, w, np.array([2, 5, 5, 8], dtype))
    assert ((L @ U) @ z.astype(F64)).tolist() == [2, 5, 5, 8]
    # [[1, 1], [1, 1]]: the second pivot is an exact zero, reported and not an error
    o2, c2, v2 = tm.from_rows([[(0, 1), (1, 1)], [(0, 1), (1, 1)]], dtype)
    w2, zp2 = im.ilu0(o2, c2, v2)
    assert w2.tolist() == [1, 1, 1, 0] and zp2 == 1
    with pytest.raises(ValueError, match="row 1 are not strictly ascending"):
        im.ilu0(*tm.from_rows([[(0, 1.0)], [(1, 1.0), (0, 1.0)]], dtype))
    with pytest.raises(ValueError, match="row 1 are not strictly ascending"):
        im.ilu0(*tm.from_rows([[(0, 1.0)], [(0, 1.0), (0, 1.0), (1, 1.0)]], dtype))
    with pytest.raises(ValueError, match="no diagonal entry stored in row 2"):
        im.ilu0(*tm.from_rows([[(0, 1.0)], [(1, 1.0)], [(0, 1.0)]], dtype))


def test_dense_pattern_is_doolittle():
    """On a fully dense pattern nothing is dropped: the factor is the LU of a plain Doolittle elimination (row by row, each
    multiplier divided first, one rounding per operation) -- in f64 bit for bit, and L U = A to the bound of the next test."""
    off, col, val = im.dense(23, F64, seed=5)
    n = 23
    A = val.reshape(n, n).copy()
    for i in range(1, n):
        for k in range(i):
            A[i, k] = A[i, k] / A[k, k]
            A[i, k + 1:] = A[i, k + 1:] - A[i, k] * A[k, k + 1:]
    w, zp = im.ilu0(off, col, val)
    assert zp is None and (bits(w) == bits(A.ravel())).all()
    assert (bits(im.ilu0(off, col, val, vector=True)[0]) == bits(w)).all()


def residual_cases(dtype):
    yield "grid 12 x 9", sg.lap2d(12, 9, dtype, seed=2, spread=1.0)
    yield "random 120", im.random_pattern(120, dtype, seed=3)
    yield "dense 70", im.dense(70, dtype, seed=3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_on_the_pattern(dtype):
    """(L U - A)_ij on every stored (i, j) within (d_ij + 2) u (|A| + |L| |U|)_ij, d_ij the number of update terms the entry
    took: each of them and the division round once (the worst case on these: 0.21 to 0.45 of the bound)."""
    u = 2.0 ** (-24 if dtype == F32 else -53)
    for what, (off, col, val) in residual_cases(dtype):
        w, zp, d = im.ilu0(off, col, val, counts=True)
        assert zp is None
        n = len(off) - 1
        L, U = im.dense_factors(off, col, w)
        A = np.zeros((n, n))
        D = np.zeros((n, n))
        rows = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
        A[rows, col.astype(np.int64)] = val.astype(F64)
        D[rows, col.astype(np.int64)] = d
        stored = np.zeros((n, n), bool)
        stored[rows, col.astype(np.int64)] = True
        err = np.abs(L @ U - A)
        bound = (D + 2) * u * (np.abs(A) + np.abs(L) @ np.abs(U))
        worst = (err[stored] / bound[stored]).max()
        print(what, np.dtype(dtype).name, "worst error / bound = %.3f" % worst)
        assert (err[stored] <= bound[stored]).all(), (what, worst)
        assert worst > 0.01  # (the bound is not vacuous)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(ic.NAMES))
def test_every_gpu_case_tells_the_wrong_variants_apart(name, dtype):
    """... and the array form of the model, which the GPU file compares against, has the scalar form's bits."""
    off, col, val = ic.matrix(name, dtype)
    want, zp = im.ilu0(off, col, val)
    got, zp_v = ic.factor(name, dtype)
    assert (bits(got) == bits(want)).all() and zp_v == zp and zp is None and np.isfinite(want).all()
    for order in im.ORDERS[1:]:
        other, _ = im.ilu0(off, col, val, order=order)
        assert (bits(other) != bits(want)).any() == (order in ic.NAMES[name]), (name, order)


@pytest.mark.parametrize("k", range(len(sg.TABLE)))
def test_body_counts(k):
    """ILU(0)-PCG needs fewer bodies than SGS-PCG in the natural ordering (34 / 40, 52 / 70, 52 / 62, 22 / 28 in the prototype's
    sequential sums) and under 0.6 of plain CG's (the recurrence with M = I) in both orderings."""
    for ordering in ("natural", "red_black"):
        off, col, val, b, tol = sg.table_case(k, ordering)
        x0 = np.zeros(len(b), val.dtype)
        w, zp = im.ilu0(off, col, val, vector=True)
        assert zp is None
        plans = (tm.Plan(off, col, tm.LOWER), tm.Plan(off, col, tm.UPPER))
        ilu = sg.sgs_pcg(off, col, val, b, x0, tol, 2000, precond=lambda r: im.ilu_apply(off, col, w, r, plans))
        cg = sg.sgs_pcg(off, col, val, b, x0, tol, 2000, precond=lambda r: r.copy())
        sgs = sg.sgs_pcg(off, col, val, b, x0, tol, 2000)
        print("table row", k, ordering, "CG", cg.iterations, "SGS", sgs.iterations, "ILU", ilu.iterations)
        assert 10 < ilu.iterations < 0.6 * cg.iterations < 1200
        if ordering == "natural":
            assert ilu.iterations < sgs.iterations
        A = np.zeros((len(b), len(b)))
        A[np.repeat(np.arange(len(b)), np.diff(off.astype(np.int64))), col.astype(np.int64)] = val.astype(F64)
        assert np.abs(A @ ilu.x.astype(F64) - b).max() < 100 * tol  # (it converged to the solution)


NEW_ENTRY_POINTS = ["smh_crs_ilu0", "smh_crs_ilu0_refactor", "smh_crs_ilu_apply_vec", "smh_pcg_ilu_solve", "smh_pcg_ilu_solve_vec"]


def test_entry_points_and_their_argument_statuses():
    """The symbols are in _lib's table and in the library; a NULL handle is SMH_ERR_INVALID before the device is needed (so this
    holds with and without one), and nothing is written through the output pointers."""
    L = sm.lib()
    for name in NEW_ENTRY_POINTS:
        assert hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes, name
        assert name in _lib.SIGNATURES
    h, zp = C.c_void_p(0x1234), C.c_size_t(77)
    assert L.smh_crs_ilu0(None, C.byref(h), C.byref(zp)) == _lib.SMH_ERR_INVALID and b"NULL" in L.smh_last_error()
    assert h.value == 0x1234 and zp.value == 77
    assert L.smh_crs_ilu0_refactor(None, None, C.byref(zp)) == _lib.SMH_ERR_INVALID and zp.value == 77
    assert L.smh_crs_ilu_apply_vec(None, None, None) == _lib.SMH_ERR_INVALID
    it, rr = C.c_size_t(5), C.c_double(3.0)
    assert L.smh_pcg_ilu_solve(None, None, None, 0, None, 0, 1e-6, 10, 0, C.byref(it), C.byref(rr)) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_ilu_solve_vec(None, None, None, None, 1e-6, 10, 0, 0, C.byref(it), C.byref(rr)) == _lib.SMH_ERR_INVALID
    assert it.value == 5 and rr.value == 3.0
    assert sm.ILUConjugateGradient(1e-6, 10, check_every=3).check_every == 3 and "ILUConjugateGradient" in dir(sm)
