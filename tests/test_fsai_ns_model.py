"""CPU: tests/fsai_ns_model.py -- the numpy restatement of the non-symmetric factorized sparse approximate inverse (two factors,
G_U G_L ~ A^-1) -- and tests/pfsai_model.py, GMRES right-preconditioned by such a pair.  A 3 x 3 case worked out by hand; on a dense
pattern G_U G_L A = I and every row solve against a dense f64 solve, within the bounds that fsai_ns_model's docstring derives from m
and the unit roundoff; on SPD matrices G_U G_L against G^T G of fsai_model.fsai; a structurally non-symmetric pattern; `singular`;
every matrix of the GPU file moving a bit under each wrong variant it can tell apart; the solver models with M^-1 as a callable; the
body counts that are the reason the preconditioner exists; and the new entry points' table entries and argument statuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bicgstab_model as bm
import fsai_cases as fc
import fsai_model as fm
import fsai_ns_cases as nc
import fsai_ns_model as nm
import gmres_model as gm
import oracle
import pbicgstab_model as pb
import pfsai_model as pf
import pgmres_model as pm
import sparsemat_amd as sm
import trisolve_model as tm
from sparsemat_amd import _lib

F32, F64 = np.float32, np.float64
DTYPES = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_worked_by_hand(dtype):
    """A = (2 1 1; 4 3 3; 8 7 9) = L U with L = (1; 2 1; 4 3 1) and U = (2 1 1; 0 1 1; 0 0 2), every step exact.  The pattern is
    dense, so the square of row i is the leading block of A (of A^T) and G_L = L^-1 = (1; -2 1; 2 -3 1), H = U^-T,
    G_U = U^-1 = (1/2 -1/2 0; 0 1 -1/2; 0 0 1/2).  Row 2 of H in full: B = A^T = (2 4 8; 1 3 7; 1 3 9); k = 0: l = (1/2, 1/2), the
    rows become (1 3) and (1 5); k = 1: l = 1, d = 5 - 3 = 2; y_2 = 1, y_1 = -(1 * 1) = -1, y_0 = -((1/2)(-1) + (1/2)(1)) = -0;
    H = y / d = (-0, -1/2, 1/2).  G_U is stored as the library's transposition leaves it: the columns of a row descending."""
    off, col, val = bm.dense_to_crs([[2, 1, 1], [4, 3, 3], [8, 7, 9]], dtype)
    gl, gu, singular = nm.fsai_ns(off, col, val)
    assert singular is None and gl[2].dtype == gu[2].dtype == dtype
    assert gl[0].tolist() == [0, 1, 3, 6] and gl[1].tolist() == [0, 0, 1, 0, 1, 2] and gl[2].tolist() == [1, -2, 1, 2, -3, 1]
    assert gu[0].tolist() == [0, 3, 5, 6] and gu[1].tolist() == [2, 1, 0, 2, 1, 2]
    assert same(gu[2], np.array([-0.0, -0.5, 0.5, -0.5, 1, 0.5], dtype))
    y, d, _ = nm.solve_row(np.array([[2, 4, 8], [1, 3, 7], [1, 3, 9]], dtype))
    assert same(y, np.array([-0.0, -1, 1], dtype)) and d == 2
    assert np.array_equal(nm.dense(*gu) @ nm.dense(*gl) @ nm.dense(off, col, val), np.eye(3))
    # a diagonal matrix: G_L = I, G_U = D^-1, one division per row; n = 1: G_U is a copy of H
    dd = np.array([4.0, 0.3, 7.0, 1e-3, 2.5e6], dtype)
    gl, gu, singular = nm.fsai_ns(np.arange(6, dtype=np.uint32), np.arange(5, dtype=np.uint32), dd)
    assert gl[2].tolist() == [1] * 5 and same(gu[2], dtype(1) / dd) and gu[1].tolist() == list(range(5)) and singular is None
    gl, gu, _ = nm.fsai_ns(*tm.from_rows([[(0, 2.5)]], dtype))
    assert gl[2].tolist() == [1] and same(gu[2], np.array([dtype(1) / dtype(2.5)])) and gu[0].tolist() == [0, 1]
    # the refusals
    with pytest.raises(ValueError, match="row 1 are not strictly ascending"):
        nm.fsai_ns(*tm.from_rows([[(0, 1.0)], [(1, 1.0), (0, 1.0)]], dtype))
    with pytest.raises(ValueError, match="no diagonal entry stored in row 2"):
        nm.fsai_ns(*tm.from_rows([[(0, 1.0)], [(1, 1.0)], [(0, 1.0)]], dtype))
    for name, (what, where) in nc.REFUSED.items():
        with pytest.raises(ValueError, match="%s %d stores more than 128" % (what, where)):
            nm.fsai_ns(*nc.matrix(name, dtype))


def exact_rows(off, col, val, transposed):
    """Per row of a factor on C = A or A^T: (J, the model's stored row -- y, or y / d of H --, the exact last row x of B^-1,
    F >= |y / d - x|, Fy >= |y - x / x_m|)."""
    c = nm.transpose_sorted(off, col, val) if transposed else (off, col, val)
    co, cc, cv = np.asarray(c[0], np.int64), np.asarray(c[1], np.int64), np.asarray(c[2])
    goff, gcol, gval, _ = nm.factor(*c, transposed)
    out = []
    for i in range(len(goff) - 1):
        J = gcol[goff[i]:goff[i + 1]].astype(np.int64)
        y, d, x, F, Fy = nm.row_bounds(nm.square(co, cc, cv, J))
        with np.errstate(all="ignore"):
            assert same(gval[goff[i]:goff[i + 1]], y / d if transposed else y)
        out.append((J, gval[goff[i]:goff[i + 1]].astype(F64), x, F, Fy))
    return out


def product_and_bound(off, col, val):
    """(G_U G_L of the model's factors, formed in f64; M* = sum_i x^U_i (x^L_i / x^L_i,m)^T of the exact rows; the bound on their
    distance; the rows): column i of G_U is H's row i against x^U_i, row i of G_L is y against x^L_i / x^L_i,m, so to first order
    |G_U G_L - M*| <= sum_i (F_i |y_i|^T + |x^U_i| Fy_i^T), taken with 1.1 for the product of two errors."""
    n = len(off) - 1
    gl, gu, singular = nm.fsai_ns(off, col, val)
    assert singular is None
    low, up = exact_rows(off, col, val, False), exact_rows(off, col, val, True)
    Mx, bound = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        (Jl, yl, xl, _, Fyl), (Ju, _, xu, Fu, _) = low[i], up[i]
        Mx[np.ix_(Ju, Jl)] += np.outer(xu, xl / xl[-1])
        bound[np.ix_(Ju, Jl)] += 1.1 * (np.outer(Fu, np.abs(yl)) + np.outer(np.abs(xu), Fyl))
    return nm.dense(*gu) @ nm.dense(*gl), Mx, bound, (low, up)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_pattern_inverts_the_matrix(dtype):
    """On a dense pattern the exact factors give G_U G_L = A^-1, so G_U G_L A - I = (G_U G_L - M*) A with M* = A^-1: within
    (sum_i F_i |y_i|^T + |x_i| Fy_i^T) |A|.  And every row solve against the dense f64 solve of its square, within F and Fy."""
    off, col, val = nc.matrix("dense70", dtype)
    n = 70
    A = nm.dense(off, col, val)
    M, Mx, bound, (low, up) = product_and_bound(off, col, val)
    u = 2.0 ** (-24 if dtype == F32 else -53)
    assert np.abs(Mx @ A - np.eye(n)).max() < 1e-12  # (the "exact" rows are exact enough to stand for A^-1)
    err, lim = np.abs(M @ A - np.eye(n)), bound @ np.abs(A) + 70 * 2.0 ** -50
    assert (err <= lim).all(), (err.max(), lim.max())
    assert err.max() > 0.01 * u and lim.max() < 1e4 * u  # (neither exact by accident nor vacuous)
    worst = 0.0
    for rows, divide in ((low, False), (up, True)):
        for J, got, x, F, Fy in rows:
            want, lim = (x, F) if divide else (x / x[-1], Fy)
            e = np.abs(got - want)
            assert (e <= lim).all(), (len(J), e.max(), lim.max())
            worst = max(worst, float(np.max(e / np.where(lim > 0, lim, 1.0))))
    print("dense70", np.dtype(dtype).name, "worst row error / bound %.3f" % worst)
    assert worst > 1e-3


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["dense70", "stored_zeros", "table1"])
def test_on_spd_matrices_the_pair_is_the_symmetric_fsai(name, dtype):
    """For a symmetric A the squares are symmetric, R(A^T, i) = R(A, i), and with x the exact last row of B^-1 both G_U G_L and
    fsai_model.fsai's G^T G approximate sum_i x_i x_i^T / x_i,m: their distance is within the sum of both bounds (fsai_model.bounds'
    row bound rb on G's rows: |G^T G - M*| <= sum_i rb_i |g_i|^T + |g_i| rb_i^T)."""
    off, col, val = fc.matrix(name, dtype)
    n = len(off) - 1
    M, Mx, bound, _ = product_and_bound(off, col, val)
    goff, gcol, gval, bad = fc.factor(name, dtype)
    assert bad is None
    G = nm.dense(goff, gcol, gval)
    for i in range(n):
        J = gcol[goff[i]:goff[i + 1]].astype(np.int64)
        _, _, g, exact, rb = fm.bounds(off, col, val, goff, gcol, i)
        ga = np.abs(g.astype(F64))
        bound[np.ix_(J, J)] += 1.1 * (np.outer(rb, ga) + np.outer(ga, rb))
    err = np.abs(M - G.T @ G)
    assert (err <= bound + 1e-300).all(), (name, err.max(), bound.max())
    assert err.max() > 0  # (two different roundings of the same thing)
    assert np.abs(M - Mx).max() <= bound.max()


@pytest.mark.parametrize("dtype", DTYPES)
def test_structurally_non_symmetric_pattern(dtype):
    """random_ns stores six columns below and three above the diagonal, chosen apart: G_L sits on the lower pattern, G_U on the upper,
    and the pattern of G_U^T is not G_L's.  The pair is still an approximate inverse: |I - G_U G_L A|_1 is under 0.5 and under half of
    Jacobi's |I - D^-1 A|_1."""
    off, col, val = nc.matrix("random_ns", dtype)
    gl, gu, singular = nc.factor("random_ns", dtype)
    n = len(off) - 1
    S = nm.dense(off, col, np.ones(len(col), dtype)) != 0
    SL, SU = nm.dense(gl[0], gl[1], np.ones(len(gl[1]))) != 0, nm.dense(gu[0], gu[1], np.ones(len(gu[1]))) != 0
    assert singular is None and np.array_equal(SL, np.tril(S)) and np.array_equal(SU, np.triu(S)) and not np.array_equal(SU.T, SL)
    assert (np.diff(gl[0].astype(np.int64)).max(), np.diff(gu[0].astype(np.int64)).max()) == (7, 4)
    assert all((np.diff(gu[1][gu[0][i]:gu[0][i + 1]].astype(np.int64)) < 0).all() for i in range(n))  # (the transposition's order)
    assert (nm.dense(*gl).diagonal() == 1).all()
    A = nm.dense(off, col, val)
    fsai, jacobi = np.linalg.norm(np.eye(n) - nm.dense(*gu) @ nm.dense(*gl) @ A, 1), np.linalg.norm(np.eye(n) - A / A.diagonal()[:, None], 1)
    print("random_ns", np.dtype(dtype).name, "|I - G_U G_L A|_1 = %.3f, |I - D^-1 A|_1 = %.3f" % (fsai, jacobi))
    assert fsai < 0.5 and fsai < 0.5 * jacobi


@pytest.mark.parametrize("dtype", DTYPES)
def test_singular(dtype):
    """A zero last pivot in row 3's square of A ((1 2; 2 4) on rows 2 and 3), which is also column 3's: G_L's row is the finite y,
    H's is y / 0.  A NaN and an Inf: the smallest row of either factor is named and the values are IEEE's."""
    rows = [[(0, 4.0)], [(1, 9.0)], [(2, 1.0), (3, 2.0)], [(2, 2.0), (3, 4.0)], [(4, 16.0)]]
    gl, gu, singular = nm.fsai_ns(*tm.from_rows(rows, dtype))
    assert singular == 3 and gl[2].tolist() == [1, 1, 1, -2, 1, 1] and np.isinf(nm.dense(*gu)[2:4, 3]).all()
    assert nm.dense(*gu).diagonal()[[0, 1, 2, 4]].tolist() == [0.25, float(dtype(1) / dtype(9)), 1.0, 0.0625]
    off, col, val = nc.matrix("random_ns", dtype)
    pos = tm.diag_positions(off, col)
    # a NaN left of row 40's diagonal: its square is the first that holds it.  An Inf on row 120's diagonal: every multiplier of that
    # pivot is x / Inf = 0 and H's entry 1 / Inf = 0 -- all values finite, and the row is still named
    v = val.copy()
    v[pos[40] - 1] = np.nan
    gl, gu, singular = nm.fsai_ns(off, col, v)
    assert singular == 40 and np.isnan(gl[2]).any() and np.isnan(gu[2]).any() and np.isfinite(gl[2]).sum() > len(gl[2]) // 2
    v = val.copy()
    v[pos[120]] = np.inf
    gl, gu, singular = nm.fsai_ns(off, col, v)
    assert singular == 120 and np.isfinite(gl[2]).all() and np.isfinite(gu[2]).all() and nm.dense(*gu)[120, 120] == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(nc.NAMES))
def test_every_gpu_case_tells_the_wrong_variants_apart(name, dtype):
    off, col, val = nc.matrix(name, dtype)
    gl, gu, singular = nc.factor(name, dtype)
    assert singular is None and np.isfinite(gl[2]).all() and np.isfinite(gu[2]).all()
    for order in nc.NAMES[name]:
        l2, u2, _ = nm.fsai_ns(off, col, val, order=order)
        assert np.array_equal(l2[1], gl[1]) and np.array_equal(u2[1], gu[1])
        assert not (same(l2[2], gl[2]) and same(u2[2], gu[2])), (name, order)
    if not nc.NAMES[name]:  # the cases of one entry per row: no variant has anything to change
        for order in nm.ORDERS[1:]:
            l2, u2, _ = nm.fsai_ns(off, col, val, order=order)
            assert same(l2[2], gl[2]) and same(u2[2], gu[2])
    lens = np.diff(gl[0].astype(np.int64))
    if name == "ragged":  # every m from 1 to 128, and around every lane width's switch to the long-row route
        assert set(lens.tolist()) == set(range(1, 129))
        assert all({nc.fit(L), nc.fit(L) + 1, L, L + 1} <= set(lens.tolist()) for L in nc.LANES)
    if name in ("arrow_row128", "arrow_col128"):  # (a row of H is a column of G_U)
        assert max(lens.max(), np.bincount(gu[1]).max()) == 128
    assert [nc.fit(L) for L in nc.LANES] == [4, 5, 8, 11, 16, 22, 32]


# ---- the solvers with M^-1 as a callable ------------------------------------------------------------------------------------------
def grid_system(g, c, dtype, scaled=False):
    """convdiff2d(g, c) with sorted rows (scaled: by 2^+-5, pgmres_model.scale_rows), a uniform right-hand side, x0 = 0, the model's
    pair as dense matrices: the products are numpy's, as in the trial the caps come from."""
    off, col, val = pm.sort_rows(*bm.convdiff2d(g, c, dtype))
    if scaled:
        val = pm.scale_rows(off, col, val)[0]
    n = g * g
    gl, gu, singular = nm.fsai_ns(off, col, val)
    assert singular is None
    A, GL, GU = nm.dense(off, col, val, dtype), nm.dense(*gl, dtype), nm.dense(*gu, dtype)
    b = np.random.default_rng(g).uniform(-1, 1, n).astype(dtype)
    return off, col, val, b, np.zeros(n, dtype), (lambda v: A @ v), (lambda v: GU @ (GL @ v)), A


@pytest.mark.parametrize("dtype", DTYPES)
def test_solver_models_from_zero_are_the_unpreconditioned_ones_on_a_after_m(dtype):
    """x does not feed back, so from x0 = 0 the bodies, cycles, estimates and rr are those of the unpreconditioned model with the
    product A o M^-1; x itself solves the system (the true residual is under 2 tol).  pfsai_model.pgmres with one callable is
    pgmres_model.pgmres bit for bit; with another one for the cycle end only x moves."""
    off, col, val, b, x0, mvp, minv, A = grid_system(12, 1.0, dtype)
    tol = 1e-8 if dtype == F64 else 1e-4
    both = lambda v: mvp(minv(v))
    got = pf.pgmres(off, col, val, b, x0, tol, 500, 10, minv, product=mvp)
    ref = pm.pgmres(off, col, val, b, x0, tol, 500, 10, minv, product=mvp)
    plain = gm.gmres(off, col, val, b, x0, tol, 500, 10, product=both)
    assert same(got.x, ref.x) and (got.iterations, got.cycles, got.breakdown, got.rr) == (ref.iterations, ref.cycles, ref.breakdown, ref.rr)
    assert (got.iterations, got.cycles, got.rr, got.estimates) == (plain.iterations, plain.cycles, plain.rr, plain.estimates) and got.cycles > 1
    assert len(got.ends) == got.cycles and not same(got.x, plain.x)
    assert np.linalg.norm(A.astype(F64) @ got.x.astype(F64) - b.astype(F64)) < 2 * tol
    other = pf.pgmres(off, col, val, b, x0, tol, 500, 10, minv, precond_end=lambda t: minv(t) * dtype(1.5), product=mvp)
    assert (other.iterations, other.cycles, other.rr, other.estimates) == (got.iterations, got.cycles, got.rr, got.estimates)
    assert not same(other.x, got.x)
    bi = pb.pbicgstab(off, col, val, b, x0, tol, 500, minv, product=mvp)
    plain = bm.bicgstab(off, col, val, b, x0, tol, 500, product=both)
    assert (bi.iterations, bi.rr, bi.breakdown) == (plain.iterations, plain.rr, plain.breakdown) and bi.converged and not same(bi.x, plain.x)
    assert np.linalg.norm(A.astype(F64) @ bi.x.astype(F64) - b.astype(F64)) < 2 * tol


# what the caps are held against: a CPU trial of the definition through these models, products dense, a random right-hand side:
# GMRES(30) 0.27 - 0.38 of the unpreconditioned bodies, BiCGSTAB 0.45 - 0.54, on the scaled rows both 0.05 - 0.11
SYSTEMS = [(24, 1.0, F64), (32, 4.0, F64), (24, 1.0, F32), (32, 4.0, F32)]


@pytest.mark.parametrize("g, c, dtype", SYSTEMS, ids=["%d-%g-%s" % (g, c, np.dtype(d).name) for g, c, d in SYSTEMS])
def test_body_counts(g, c, dtype):
    """To tol 1e-8 (f64) / 1e-4 (f32) from x0 = 0: FSAI-GMRES(30) needs at most 0.5 of GMRES(30)'s bodies and FSAI-BiCGSTAB at most
    0.65 of BiCGSTAB's."""
    off, col, val, b, x0, mvp, minv, A = grid_system(g, c, dtype)
    tol = 1e-8 if dtype == F64 else 1e-4
    g0 = pm.pgmres(off, col, val, b, x0, tol, 3000, 30, pm.identity, product=mvp)
    g1 = pm.pgmres(off, col, val, b, x0, tol, 3000, 30, minv, product=mvp)
    b0 = pb.pbicgstab(off, col, val, b, x0, tol, 3000, pm.identity, product=mvp)
    b1 = pb.pbicgstab(off, col, val, b, x0, tol, 3000, minv, product=mvp)
    print("convdiff2d(%d, %g)" % (g, c), np.dtype(dtype).name, "GMRES(30)", g0.iterations, "->", g1.iterations, "BiCGSTAB", b0.iterations, "->", b1.iterations)
    assert g1.estimates[-1] < tol and g0.estimates[-1] < tol and b1.converged and b0.converged
    assert 10 < g1.iterations <= 0.5 * g0.iterations, (g0.iterations, g1.iterations)
    assert 10 < b1.iterations <= 0.65 * b0.iterations, (b0.iterations, b1.iterations)


@pytest.mark.parametrize("dtype", DTYPES)
def test_body_counts_on_scaled_rows(dtype):
    """convdiff2d(24, 1.0) with its rows scaled by 2^+-5: the pair undoes the scaling as Jacobi does (G_U carries 1 / d), and both
    solvers need at most 0.2 of the unpreconditioned bodies."""
    off, col, val, b, x0, mvp, minv, A = grid_system(24, 1.0, dtype, scaled=True)
    tol = 1e-8 if dtype == F64 else 1e-4
    g0 = pm.pgmres(off, col, val, b, x0, tol, 3000, 30, pm.identity, product=mvp)
    g1 = pm.pgmres(off, col, val, b, x0, tol, 3000, 30, minv, product=mvp)
    b0 = pb.pbicgstab(off, col, val, b, x0, tol, 3000, pm.identity, product=mvp)
    b1 = pb.pbicgstab(off, col, val, b, x0, tol, 3000, minv, product=mvp)
    print("scaled rows", np.dtype(dtype).name, "GMRES(30)", g0.iterations, "->", g1.iterations, "BiCGSTAB", b0.iterations, "->", b1.iterations)
    # (the unpreconditioned BiCGSTAB may end on a breakdown before tol in f32: fewer bodies than it would need, so the cap only gets harder)
    assert g1.estimates[-1] < tol and g0.estimates[-1] < tol and b1.converged
    assert 10 < g1.iterations <= 0.2 * g0.iterations and 10 < b1.iterations <= 0.2 * b0.iterations


# ---- the bindings -------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = ["smh_crs_fsai_ns", "smh_crs_fsai_ns_apply_vec", "smh_gmres_fsai_solve", "smh_gmres_fsai_solve_vec", "smh_bicgstab_fsai_solve",
                    "smh_bicgstab_fsai_solve_vec"]


def test_header_and_table_declare_the_entry_points():
    """The header lists the names among the additions made without a version change (before the ABI define, which stays 3) and
    declares each once; _lib.SIGNATURES has them with the argument counts of the declarations; PRECONDS keeps its four keys."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sparsemat_hip.h")).read()
    head, define, rest = text.partition("#define SMH_ABI_VERSION 3")
    assert define
    L = sm.lib()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\b" % name, head), name
        decl = re.findall(r"^int %s\(([^;]*)\);" % name, rest, re.M)
        assert len(decl) == 1, name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == decl[0].count(",") + 1, name
        assert getattr(L, name).argtypes == args
    assert L.smh_abi_version() == 3
    assert list(_lib.PRECONDS) == [None, "jacobi", "sgs", "ilu"] and _lib.PRECOND_NAMES == (None, "jacobi", "sgs", "ilu", "fsai")
    for cls in (sm.GMRES, sm.BiCGStab):
        s = cls(1e-6, 10, precond="fsai")
        assert s.precond == "fsai" and s.singular is None and s.factor is None
        with pytest.raises(ValueError):
            cls(1e-6, 10, precond="amg")


def test_argument_statuses_need_no_device():
    """A NULL handle is SMH_ERR_INVALID before the device is needed, and nothing is written through the output pointers."""
    L = sm.lib()
    gl, gu, bad = C.c_void_p(0x1234), C.c_void_p(0x5678), C.c_size_t(77)
    assert L.smh_crs_fsai_ns(None, C.byref(gl), C.byref(gu), C.byref(bad)) == _lib.SMH_ERR_INVALID and b"NULL" in L.smh_last_error()
    assert gl.value == 0x1234 and gu.value == 0x5678 and bad.value == 77
    assert L.smh_crs_fsai_ns_apply_vec(None, None, None, None) == _lib.SMH_ERR_INVALID
    it, rr, cy, brk = C.c_size_t(5), C.c_double(3.0), C.c_size_t(9), C.c_int(-4)
    outs = (C.byref(it), C.byref(rr))
    assert L.smh_gmres_fsai_solve(None, None, None, None, 0, None, 0, 1e-6, 10, 30, 0, *outs, C.byref(cy), C.byref(brk)) == _lib.SMH_ERR_INVALID
    assert L.smh_gmres_fsai_solve_vec(None, None, None, None, None, 1e-6, 10, 30, 0, 0, *outs, C.byref(cy), C.byref(brk)) == _lib.SMH_ERR_INVALID
    assert L.smh_bicgstab_fsai_solve(None, None, None, None, 0, None, 0, 1e-6, 10, 0, *outs, C.byref(brk)) == _lib.SMH_ERR_INVALID
    assert L.smh_bicgstab_fsai_solve_vec(None, None, None, None, None, 1e-6, 10, 0, 0, *outs, C.byref(brk)) == _lib.SMH_ERR_INVALID
    assert (it.value, rr.value, cy.value, brk.value) == (5, 3.0, 9, -4)


def test_without_a_device_the_entry_points_refuse():
    """With no HIP device visible no handle can be made, so the way to the factors and to the solvers ends in SMH_ERR_NO_DEVICE, never
    in a fallback.  (With a device this checks nothing and the GPU files do.)"""
    n = C.c_int(0)
    sm.lib().smh_device_count(C.byref(n))
    if n.value > 0:
        return
    with pytest.raises(_lib.SparseMatPanic) as e:
        sm.SparseMatCRS.from_raw_parts(2, 2, [0, 1, 2], [0, 1], np.ones(2, F32)).fsai_ns()
    assert e.value.status == _lib.SMH_ERR_NO_DEVICE
    for cls in (sm.GMRES, sm.BiCGStab):
        with pytest.raises(_lib.SparseMatPanic) as e:
            cls(1e-6, 10, precond="fsai").solve(sm.SparseMatCRS.from_raw_parts(2, 2, [0, 1, 2], [0, 1], np.ones(2, F32)), np.ones(2, F32), np.zeros(2, F32))
        assert e.value.status == _lib.SMH_ERR_NO_DEVICE
