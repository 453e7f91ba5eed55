"""CPU: tests/sgs_model.py -- the numpy restatement of the symmetric Gauss-Seidel preconditioner and of its CG.  The application
inverts M = (D + L) D^-1 (D + U); with M = I forced the recurrence is cg_model's CG; the body counts of the four grid cases
stay under 0.6 of Jacobi's (the reason the preconditioner exists), in the natural and in the red-black ordering; b = 0 and
iter_max = 0 behave like the reference's loop."""
import numpy as np
import pytest

import cg_model
import sgs_model as sg
import trisolve_model as tm

F32, F64 = np.float32, np.float64


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def dense(off, col, val):
    n = len(off) - 1
    A = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(np.asarray(off, np.int64)))
    np.add.at(A, (rows, np.asarray(col, np.int64)), np.asarray(val, np.float64))
    return A


def test_generators():
    off, col, val = sg.lap2d(5, 4, F64, seed=3, spread=2.0)
    A = dense(off, col, val)
    assert (A == A.T).all() and np.allclose(A.sum(1), 0.05) and np.linalg.eigvalsh(A).min() > 0.04
    rows = np.repeat(np.arange(20), np.diff(off.astype(np.int64)))
    assert all((np.diff(col[off[i]:off[i + 1]].astype(np.int64)) > 0).all() for i in range(20))  # columns ascending
    w = -A[np.triu_indices(20, 1)]
    w = w[w > 0]
    assert len(w) == 4 * 4 + 5 * 3 and 0.1 <= w.min() and w.max() <= 10.0
    assert (sg.lap2d(5, 4, F64)[2][col != rows] == -1.0).all()  # spread 0: unit weights
    p = sg.red_black(3, 4)
    assert p.tolist() == [0, 2, 5, 7, 8, 10, 1, 3, 4, 6, 9, 11]  # stable: (i + j) even first, each colour in index order
    o, c, v = sg.permute_symmetric(off, col, val, sg.red_black(5, 4))
    P = np.eye(20)[sg.red_black(5, 4)]
    assert (dense(o, c, v) == P @ A @ P.T).all()


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("ordering", ["natural", "red_black"])
def test_apply_inverts_m(dtype, ordering):
    """M z recomputed in f64 equals r.  Each of the two substitutions is backward stable row by row (at most 2 strict entries in
    a row of a triangle of the five-point grid, 4 after the red-black renumbering: gamma_6 covers products, subtractions, the
    scaling and the division), so |M z - r| <= 3 gamma_6 (|D + L| |D^-1| |D + U|) |z| componentwise to first order; 1.1 for
    the second order."""
    off, col, val, r, _ = sg.table_case(3 if dtype == F32 else 1, ordering)
    z = sg.sgs_apply(off, col, val, r)
    plans = (tm.Plan(off, col, tm.LOWER), tm.Plan(off, col, tm.UPPER))
    assert (bits(sg.sgs_apply(off, col, val, r, plans)) == bits(z)).all()
    A = dense(off, col, val)
    D, L, U = np.diag(np.diag(A)), np.tril(A, -1), np.triu(A, 1)
    M = (D + L) @ np.diag(1.0 / np.diag(A)) @ (D + U)
    u = 2.0 ** (-24 if dtype == F32 else -53)
    bound = 1.1 * 3 * (6 * u) * (np.abs(D + L) @ np.diag(1.0 / np.diag(A)) @ np.abs(D + U)) @ np.abs(z.astype(np.float64))
    assert (np.abs(M @ z.astype(np.float64) - r.astype(np.float64)) <= bound).all()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_identity_preconditioner_is_plain_cg(dtype):
    off, col, val, b, tol = sg.table_case(3 if dtype == F32 else 0, "natural")
    x0 = np.zeros(len(b), dtype)
    want = cg_model.cg(off, col, val, b, x0, tol, 1000, mode="sequential")
    got = sg.sgs_pcg(off, col, val, b, x0, tol, 1000, mode="sequential", precond=lambda r: r.copy())
    assert 20 < want.iterations < 1000 and got.iterations == want.iterations
    assert (bits(got.x) == bits(want.x)).all() and bits(np.array([got.rr])) == bits(np.array([want.rr]))


@pytest.mark.parametrize("k", range(len(sg.TABLE)))
def test_body_counts_stay_under_six_tenths_of_jacobi(k):
    """(24 x 17, 0, f64): Jacobi 111, SGS 40 natural / 55 red-black; (24 x 17, 2, f64): 170 / 168 (the renumbered Jacobi sums in
    another order), 70, 84; (40 x 33, 1, f64): 165, 62, 83; (24 x 17, 1, f32, 1e-4): 71 / 67, 28, 34 -- sequential sums; the
    device's trees move a count by a body or two."""
    counts = {}
    for ordering in ("natural", "red_black"):
        off, col, val, b, tol = sg.table_case(k, ordering)
        x0 = np.zeros(len(b), val.dtype)
        jac = cg_model.pcg(off, col, val, b, x0, tol, 2000)
        sgs = sg.sgs_pcg(off, col, val, b, x0, tol, 2000)
        counts[ordering] = (jac.iterations, sgs.iterations)
        assert 10 < sgs.iterations < 0.6 * jac.iterations < 1200, (k, ordering, counts)
        A = dense(off, col, val)
        assert np.abs(A @ sgs.x.astype(np.float64) - b).max() < 100 * tol  # (it converged to the solution)
    print("table row", k, counts)
    assert counts["natural"][1] < counts["red_black"][1]  # fewer levels cost bodies: the trade the ordering makes


@pytest.mark.parametrize("mode", ["sequential", "device"])
def test_zero_right_hand_side_and_iter_max_zero(mode):
    off, col, val, b, tol = sg.table_case(0, "natural")
    n = len(b)
    # b = 0 from x = 0: alpha = 0 / 0, the stop test never fires on a NaN: the loop runs to iter_max, like the reference's
    zero = sg.sgs_pcg(off, col, val, np.zeros(n), np.zeros(n), tol, 7, mode=mode)
    ref = cg_model.pcg(off, col, val, np.zeros(n), np.zeros(n), tol, 7, mode=mode)
    assert zero.iterations == ref.iterations == 7 and np.isnan(zero.x).all() and np.isnan(zero.rr)
    # iter_max = 0: no body; x untouched, r.r the initial residual's
    x0 = np.linspace(-1, 1, n)
    none = sg.sgs_pcg(off, col, val, b, x0, tol, 0, mode=mode)
    assert none.iterations == 0 and (bits(none.x) == bits(x0)).all() and none.rr == none.rr0 > 0
