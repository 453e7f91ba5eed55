"""CPU: tests/fsai_model.py -- the numpy restatement of the factorized sparse approximate inverse and of its application.  Two cases
worked out by hand, the dense pattern against the model's own LDL^T, the two bounds of the model's docstring on every matrix of the
GPU file, every such matrix moving a bit under each wrong variant it can tell apart, the body counts that are the reason the
preconditioner exists, and the new entry points' table entries and argument statuses (which need no device)."""
import ctypes as C

import numpy as np
import pytest

import cg_model
import fsai_cases as fc
import fsai_model as fm
import oracle
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
    """tridiag(2, -1) of 3 rows.  Row 0: B = (2), G = 1 / sqrt(2).  Rows 1 and 2: B = (2; -1 2): l = -1 / 2, the last pivot is
    2 - (-0.5)(-1) = 1.5, y = (0.5, 1), g = 1 / sqrt(1.5), G = (0.5 g, g) -- the halving is exact.  And a diagonal matrix:
    G = D^(-1/2), one square root and one division per row."""
    T = dtype
    off, col, val = tm.from_rows([[(0, 2), (1, -1)], [(0, -1), (1, 2), (2, -1)], [(1, -1), (2, 2)]], dtype)
    goff, gcol, gval, bad = fm.fsai(off, col, val)
    g = T(1) / np.sqrt(T(1.5))
    assert goff.tolist() == [0, 1, 3, 5] and gcol.tolist() == [0, 0, 1, 1, 2] and bad is None and gval.dtype == dtype
    assert (bits(gval) == bits(np.array([T(1) / np.sqrt(T(2)), T(0.5) * g, g, T(0.5) * g, g], dtype))).all()
    toff, tcol, tval = fm.transpose(goff, gcol, gval)
    assert toff.tolist() == [0, 2, 4, 5] and tcol.tolist() == [1, 0, 2, 1, 2]  # (the reference's transposition prepends)
    assert (bits(tval) == bits(gval[[1, 0, 3, 2, 4]])).all()
    d = np.array([4.0, 0.3, 7.0, 1e-3, 2.5e6], dtype)
    goff, gcol, gval, bad = fm.fsai(np.arange(6, dtype=np.uint32), np.arange(5, dtype=np.uint32), d)
    assert goff.tolist() == list(range(6)) and gcol.tolist() == list(range(5)) and bad is None
    assert (bits(gval) == bits(np.array([T(1) / np.sqrt(x) for x in d], dtype))).all() and gval[0] == 0.5
    # not positive definite: the row is named, its values are IEEE's; a refused pattern; a row beyond the limit
    assert fm.fsai(*tm.from_rows([[(0, 1), (1, 2)], [(0, 2), (1, 1)]], dtype))[3] == 1
    assert fm.fsai(*tm.from_rows([[(0, 1)], [(1, 0)]], dtype))[2].tolist() == [1, np.inf]
    with pytest.raises(ValueError, match="row 1 are not strictly ascending"):
        fm.fsai(*tm.from_rows([[(0, 1.0)], [(1, 1.0), (0, 1.0)]], dtype))
    with pytest.raises(ValueError, match="no diagonal entry stored in row 2"):
        fm.fsai(*tm.from_rows([[(0, 1.0)], [(1, 1.0)], [(0, 1.0)]], dtype))
    for name, row in fc.REFUSED.items():
        with pytest.raises(ValueError, match="row %d stores more than 128" % row):
            fm.fsai(*fc.matrix(name, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_pattern_is_the_last_rows_of_the_ldlt(dtype):
    """On a dense SPD pattern the triangle of row i is the leading block of A, whose elimination is the first i steps of A's own: row
    i of G is the back substitution on the leading block of ONE factorization L D L^T of A, scaled -- bit for bit."""
    n = 23
    off, col, val = fc.dense(n, dtype, seed=5)
    A = val.reshape(n, n)
    F = fm.eliminate(np.tril(A))
    goff, gcol, gval, bad = fm.fsai(off, col, val)
    assert bad is None and goff.tolist() == [i * (i + 1) // 2 for i in range(n + 1)]
    T = dtype
    for i in range(n):
        y = np.zeros(i + 1, dtype)
        y[i] = 1
        for p in range(i - 1, -1, -1):
            s = T(0)
            for q in range(p + 1, i + 1):
                s = T(s + T(F[q, p] * y[q]))
            y[p] = -s
        row = y * T(T(1) / np.sqrt(F[i, i]))
        assert (bits(row) == bits(gval[goff[i]:goff[i + 1]])).all(), i


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [k for k in fc.NAMES if k != "empty"])
def test_bounds_on_every_gpu_case(name, dtype):
    """diag(G A G^T) - 1 and the distance of G from a dense f64 solve of B x = e_m, row by row within the bounds that
    fsai_model's docstring derives from the row's operation count (rows beyond 400: every seventh)."""
    off, col, val = fc.matrix(name, dtype)
    goff, gcol, gval, bad = fc.factor(name, dtype)
    assert bad is None
    n = len(off) - 1
    worst = [0.0, 0.0]
    for i in range(0, n, 1 if n <= 400 else 7):
        diag, diag_bound, g, exact, row_bound = fm.bounds(off, col, val, goff, gcol, i)
        assert (bits(g) == bits(gval[goff[i]:goff[i + 1]])).all()
        err = np.abs(g.astype(F64) - exact)
        assert abs(diag - 1.0) <= diag_bound, (name, i, diag - 1.0, diag_bound)
        assert (err <= row_bound).all(), (name, i, err, row_bound)
        ratio = np.divide(err, row_bound, out=np.zeros_like(err), where=row_bound > 0)  # (a stored zero gives an exact 0 within a bound of 0)
        worst = [max(worst[0], abs(diag - 1.0) / diag_bound), max(worst[1], ratio.max())]
    print(name, np.dtype(dtype).name, "worst error / bound: diag %.3f, row %.3f" % tuple(worst))
    if name in ("dense70", "ragged", "lap3d12"):
        assert worst[0] > 1e-3 and worst[1] > 1e-3  # (the bounds are not vacuous)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(fc.NAMES))
def test_every_gpu_case_tells_the_wrong_variants_apart(name, dtype):
    off, col, val = fc.matrix(name, dtype)
    goff, gcol, want, bad = fc.factor(name, dtype)
    assert bad is None and np.isfinite(want).all()
    for order in fm.ORDERS[1:]:
        if order == "upper" and name != "nonsymmetric":
            continue  # (the other cases are symmetric: their upper triangle is the lower's mirror image)
        other = fm.fsai(off, col, val, order=order)[2]
        assert (bits(other) != bits(want)).any() == (order in fc.NAMES[name]), (name, order)
    if name not in ("empty", "nonsymmetric"):
        assert (bits(fm.fsai(off, col, val, order="upper")[2]) == bits(want)).all()


def model_precond(g):
    gt = fm.transpose(*g)
    return lambda r: fm.fsai_apply(g, gt, r, oracle.spmv)


def test_identity_factor_gives_cg():
    """The FSAI of the identity is the identity, and FSAI-PCG with it is the recurrence with z = r: plain CG's bits."""
    off, col, val, b, tol = sg.table_case(1, "natural")
    n = len(b)
    eye = np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, val.dtype)
    g = fm.fsai(*eye)
    assert g[3] is None and all(np.array_equal(x, y) for x, y in zip(g[:3], eye))
    x0 = np.zeros(n, val.dtype)
    got = sg.sgs_pcg(off, col, val, b, x0, tol, 40, precond=model_precond(g[:3]))
    want = sg.sgs_pcg(off, col, val, b, x0, tol, 40, precond=lambda r: r.copy())
    assert got.iterations == want.iterations == 40 and (bits(got.x) == bits(want.x)).all() and got.rr == want.rr


@pytest.mark.parametrize("k", range(len(sg.TABLE)))
def test_body_counts(k):
    """FSAI-PCG needs at most 0.6 of Jacobi-PCG's bodies (cg_model.pcg) in both orderings -- 0.48 to 0.54 in a sequential prototype,
    the same in either ordering -- and reaches the solution: the true residual is below 2 tol."""
    for ordering in ("natural", "red_black"):
        off, col, val, b, tol = sg.table_case(k, ordering)
        n = len(b)
        x0 = np.zeros(n, val.dtype)
        g = fc.factor("table%d%s" % (k, "-rb" if ordering == "red_black" else ""), val.dtype)
        fsai = sg.sgs_pcg(off, col, val, b, x0, tol, 2000, precond=model_precond(g[:3]))
        jac = cg_model.pcg(off, col, val, b, x0, tol, 2000)
        print("table row", k, ordering, "Jacobi", jac.iterations, "FSAI", fsai.iterations)
        assert 10 < fsai.iterations <= 0.6 * jac.iterations < 1200
        A = np.zeros((n, n))
        A[np.repeat(np.arange(n), np.diff(off.astype(np.int64))), col.astype(np.int64)] = val.astype(F64)
        assert np.linalg.norm(A @ fsai.x.astype(F64) - b.astype(F64)) < 2 * tol


NEW_ENTRY_POINTS = ["smh_crs_fsai", "smh_crs_fsai_apply_vec", "smh_pcg_fsai_solve", "smh_pcg_fsai_solve_vec"]


def test_entry_points_and_their_argument_statuses():
    """The symbols are in _lib's table and in the library; a NULL handle is SMH_ERR_INVALID before the device is needed (so this
    holds with and without one), and nothing is written through the output pointers."""
    L = sm.lib()
    for name in NEW_ENTRY_POINTS:
        assert hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes, name
        assert name in _lib.SIGNATURES
    g, gt, bad = C.c_void_p(0x1234), C.c_void_p(0x5678), C.c_size_t(77)
    assert L.smh_crs_fsai(None, C.byref(g), C.byref(gt), C.byref(bad)) == _lib.SMH_ERR_INVALID and b"NULL" in L.smh_last_error()
    assert g.value == 0x1234 and gt.value == 0x5678 and bad.value == 77
    assert L.smh_crs_fsai_apply_vec(None, None, None, None) == _lib.SMH_ERR_INVALID
    it, rr = C.c_size_t(5), C.c_double(3.0)
    assert L.smh_pcg_fsai_solve(None, None, None, None, 0, None, 0, 1e-6, 10, 0, C.byref(it), C.byref(rr)) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_fsai_solve_vec(None, None, None, None, None, 1e-6, 10, 0, 0, C.byref(it), C.byref(rr)) == _lib.SMH_ERR_INVALID
    assert it.value == 5 and rr.value == 3.0
    s = sm.FSAIConjugateGradient(1e-6, 10, check_every=3)
    assert s.check_every == 3 and s.factor is None and "FSAIConjugateGradient" in dir(sm)


def test_without_a_device_the_entry_points_refuse():
    """With no HIP device visible no handle can be made, so the way to the factorization ends in SMH_ERR_NO_DEVICE, never in a
    fallback; the NULL statuses above need no device.  (With a device this checks nothing and the GPU file does.)"""
    n = C.c_int(0)
    sm.lib().smh_device_count(C.byref(n))
    if n.value > 0:
        return
    with pytest.raises(_lib.SparseMatPanic) as e:
        sm.SparseMatCRS.from_raw_parts(2, 2, [0, 1, 2], [0, 1], np.ones(2, F32)).fsai()
    assert e.value.status == _lib.SMH_ERR_NO_DEVICE
