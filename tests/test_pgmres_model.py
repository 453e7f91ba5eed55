"""CPU: tests/pgmres_model.py -- the contract of the right-preconditioned GMRES (smh_gmres_precond_solve*, gmres.hip).  With the
identity it is gmres_model.gmres but for the two sums of x; from x0 = 0 it is gmres_model.gmres on the product A o M^-1; on the
convection-diffusion grids the triangular preconditioners, and on badly scaled rows Jacobi, cut the bodies to a fraction; the true
residual of its x is the one the stop rule promises; every case of the GPU file moves a bit under each wrong variant of the
arithmetic it can tell apart; the binding and the header declare the two entry points."""
import os
import re

import numpy as np
import pytest

import bicgstab_model as bm
import gmres_cases
import gmres_model as gm
import ilu_model as im
import oracle
import pgmres_cases as pc
import pgmres_model as pm
import sparsemat_amd as sm
from sparsemat_amd import _lib
from test_gmres_model import true_residual

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
IDS = ["f32", "f64"]


def same(a, b):
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]) and np.array_equal(np.signbit(a[~na]), np.signbit(b[~nb])))


def bits(r):
    return r.x.tobytes(), r.iterations, r.cycles, r.rr.tobytes(), r.breakdown


# ---- 1: the identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_identity_is_gmres_but_for_the_sums_of_x(dtype):
    """On gmres_cases.BIT_CASES: bodies, cycles, the code, every estimate, rr and the last basis are gmres_model.gmres's bit for bit
    (x does not feed back: the residual is rebuilt from the basis).  x differs in the ORDER of one sum per cycle end.  Both orders
    add the same j rounded products v_c y_c to x with j additions -- gmres (..(x + p_0) + ..) + p_{j-1}, this model
    x + ((p_0 + p_1) .. + p_{j-1}) -- so each result is off from the exact sum x + sum p_c by at most gamma_j (|x| + sum |p_c|),
    gamma_j = j u / (1 - j u) (Higham, Accuracy and Stability, section 4.2: any order of j additions), element by element.  The two
    x entering a cycle end differ by the bound e so far, which both carry along: e' = e + 2 gamma_j (|x| + e + sum |p_c|)."""
    u = np.finfo(dtype).eps / 2
    for case in gmres_cases.BIT_CASES:
        off, col, val, b, x0 = case.system(dtype)
        want = gm.gmres(off, col, val, b, x0, case.tol(dtype), case.iter_max, case.restart)
        got = pm.pgmres(off, col, val, b, x0, case.tol(dtype), case.iter_max, case.restart, pm.identity)
        assert (got.iterations, got.cycles, got.breakdown) == (want.iterations, want.cycles, want.breakdown), case.name
        assert same(np.array(got.estimates), np.array(want.estimates)) and same(got.rr, want.rr) and same(got.rr0, want.rr0), case.name
        assert len(got.basis) == len(want.basis) and all(same(p, q) for p, q in zip(got.basis, want.basis)), case.name
        e = np.zeros(case.n)
        for j, x_before, terms, _ in got.x_sums:
            gamma = j * u / (1 - j * u)
            e = e + 2 * gamma * (x_before + e + terms)
        finite = np.isfinite(want.x)
        assert np.array_equal(finite, np.isfinite(got.x)), case.name
        diff = np.abs(got.x.astype(F64) - want.x.astype(F64))[finite]
        assert (diff <= e[finite]).all(), (case.name, diff.max(), e[finite].max())
        if want.iterations == 0:
            assert same(got.x, want.x) and same(got.x, np.asarray(x0, dtype))


# ---- 2 - 5: the issue's table ----------------------------------------------------------------------------------------------------
TABLE = [(24, 1.0), (32, 4.0)]
TOLS = {F32: 1e-3, F64: 1e-8}
_TABLE = {}


def table_system(g, c, dtype, scaled=False):
    """convdiff2d(g, c) with sorted rows, b = A x* (x* uniform in [-1, 1)); scaled: row i times 2^k_i, b = (the scaled A) x*"""
    key = g, c, np.dtype(dtype).name, scaled
    if key not in _TABLE:
        off, col, val = pm.sort_rows(*bm.convdiff2d(g, c, dtype))
        if scaled:
            val, _ = pm.scale_rows(off, col, val)
        x_star = np.random.default_rng(g).uniform(-1, 1, g * g).astype(dtype)
        _TABLE[key] = off, col, val, oracle.spmv(off, col, val, x_star)
    return _TABLE[key]


def preconds(off, col, val):
    w, zp = im.ilu0(off, col, val, vector=True)
    assert zp is None
    return {"jacobi": pm.jacobi(off, col, val), "sgs": pm.sgs(off, col, val), "ilu": pm.ilu(off, col, w)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("g,c", TABLE)
def test_table_bodies_and_true_residual(g, c, dtype):
    """From x0 = 0, restart 30 and 10, to tol: (2) bodies, cycles, estimates and rr of every kind are gmres_model.gmres's on the
    product A o M^-1, bit for bit; (3) ILU(0) takes at most 0.30 and SGS at most 0.35 of the unpreconditioned bodies; (5) the true
    residual of x, formed in f64, is below 2 tol."""
    off, col, val, b = table_system(g, c, dtype)
    n, tol = g * g, TOLS[dtype]
    x0 = np.zeros(n, dtype)
    ms = preconds(off, col, val)
    A = lambda v: oracle.spmv(off, col, val, v)
    for restart in (30, 10):
        plain = gm.gmres(off, col, val, b, x0, tol, 4000, restart)
        assert plain.iterations < 4000 and plain.estimates[-1] < tol
        counts = {}
        for kind, M in ms.items():
            got = pm.pgmres(off, col, val, b, x0, tol, 4000, restart, M)
            ref = gm.gmres(off, col, val, b, x0, tol, 4000, restart, product=lambda v: A(M(v)))
            assert (got.iterations, got.cycles, got.breakdown) == (ref.iterations, ref.cycles, ref.breakdown) and got.breakdown == 0
            assert same(np.array(got.estimates), np.array(ref.estimates)) and same(got.rr, ref.rr)
            assert got.estimates[-1] < tol
            true = true_residual(off, col, val, b, got.x)
            print(g, c, np.dtype(dtype).name, restart, kind, got.iterations, "of", plain.iterations, "true/tol", true / tol)
            assert true < 2 * tol, (kind, restart, true)
            counts[kind] = got.iterations
        assert counts["ilu"] <= 0.30 * plain.iterations, (restart, counts, plain.iterations)
        assert counts["sgs"] <= 0.35 * plain.iterations, (restart, counts, plain.iterations)
        assert counts["jacobi"] == plain.iterations  # (a constant diagonal: Jacobi changes nothing but a scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_jacobi_on_scaled_rows(dtype):
    """(4) convdiff2d(24, 1.0) with row i scaled by 2^k_i, k in -5 .. 5: Jacobi takes at most 0.25 of the unpreconditioned bodies,
    equals gmres_model.gmres on A o M^-1 bit for bit, and its true residual is below 2 tol."""
    off, col, val, b = table_system(24, 1.0, dtype, scaled=True)
    tol, x0 = TOLS[dtype], np.zeros(576, dtype)
    M = pm.jacobi(off, col, val)
    A = lambda v: oracle.spmv(off, col, val, v)
    for restart in (30, 10):
        plain = gm.gmres(off, col, val, b, x0, tol, 6000, restart)
        got = pm.pgmres(off, col, val, b, x0, tol, 6000, restart, M)
        ref = gm.gmres(off, col, val, b, x0, tol, 6000, restart, product=lambda v: A(M(v)))
        assert plain.iterations < 6000 and plain.estimates[-1] < tol and got.estimates[-1] < tol
        assert (got.iterations, got.cycles, got.breakdown) == (ref.iterations, ref.cycles, ref.breakdown)
        assert same(np.array(got.estimates), np.array(ref.estimates)) and same(got.rr, ref.rr)
        true = true_residual(off, col, val, b, got.x)
        print(np.dtype(dtype).name, restart, got.iterations, "of", plain.iterations, "true/tol", true / tol)
        assert got.iterations <= 0.25 * plain.iterations, (restart, got.iterations, plain.iterations)
        assert true < 2 * tol, (restart, true)


# ---- 6: what the bit comparisons of the GPU file can tell apart --------------------------------------------------------------------
def can_tell(case, wrong, want):
    """Which wrong variants a case of the GPU file must move under.  Nothing shows on the exact and the all-NaN cases or without a
    body.  "reciprocal" and "fma" are Jacobi's alone (the other kinds apply no division of their own, and x + q is one addition).
    "x first" needs a cycle end with two columns: restart 1 has none (t = v_0 y_0 then M^-1: the same operations).  The sizes
    n <= 3 are there for the kernels' edge paths (a Krylov space exhausted after n bodies, sums of a handful of terms)."""
    if case.exact or want.iterations == 0 or wrong in case.blind:
        return False
    if wrong in ("reciprocal", "fma") and case.kind != "jacobi":
        return False
    if wrong == "x first" and case.restart == 1:
        return False
    return case.n > 3


# per variant, a case that tells it (asserted below among all the others)
NAMED = {"left": "sgs convdiff2d(12, 1.0) natural, restart 5, iter_max 12", "x first": "ilu convdiff2d(24, 1.0) red_black, restart 30, to tol",
         "reciprocal": "jacobi n=259", "fma": "jacobi restart=8"}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", pc.KINDS)
def test_gpu_cases_move_under_every_wrong_variant(kind, dtype):
    moved = set()
    for case in [c for c in pc.BIT_CASES if c.kind == kind]:
        want = case.model(dtype)
        for wrong in pm.WRONG[1:]:
            if wrong in ("reciprocal", "fma") and kind != "jacobi":
                continue
            other = case.model(dtype, wrong=wrong)
            if can_tell(case, wrong, want):
                assert bits(other) != bits(want), (case.name, wrong)
                moved.add((case.name, wrong))
        seq = case.model(dtype, mode="sequential")
        if not case.exact and want.iterations and case.n > 5:
            assert bits(seq) != bits(want), (case.name, "sequential sums")
    for wrong, name in NAMED.items():
        if name.startswith(kind):
            assert (name, wrong) in moved, (wrong, name)


def test_the_cases_are_what_their_names_say():
    for dtype in DTYPES:
        for case in pc.JACOBI:
            want = case.model(dtype)
            if case in pc.J_SIZES and case.n > 3:
                assert (want.iterations, want.cycles, want.breakdown) == (8, 3, 0), case.name
            if case in pc.J_RESTARTS:
                assert want.iterations == 2 * case.restart + 2 and want.cycles >= 3 and want.breakdown == 0, (case.name, want.cycles)
        zero = pc.J_SIZES[0].model(dtype)
        assert (zero.iterations, zero.cycles, zero.breakdown) == (0, 0, 2)
        stop = pc.J_STOPS[0].model(dtype)
        k = stop.iterations
        assert 3 < k < 30 and k % 8 and k % 3 and stop.cycles == 1 and stop.estimates[-1] < pc.J_STOPS[0].tol(dtype) <= min(stop.estimates[:-1]), k
        assert [c.model(dtype).cycles for c in pc.J_STOPS[1:]] == [3, 2]
        d = pc.J_SPECIAL[0].model(dtype)
        assert (d.iterations, d.cycles, d.breakdown, float(d.rr)) == (1, 1, 1, 0.0) and d.x.tolist() == [0, 0, 0, 1.5, 0, 0, 0]
        assert len(set(pc.J_SPECIAL[0].system(dtype)[2].tolist())) == 5
        nan = pc.J_SPECIAL[2].model(dtype)
        assert (nan.iterations, nan.cycles, nan.breakdown) == (7, 3, 0) and np.isnan(nan.x).all()
        for case in pc.SGS + pc.ILU:
            want = case.model(dtype)
            if case.restart == 5:
                assert (want.iterations, want.cycles, want.breakdown) == (12, 3, 0), case.name
            else:
                # (the red-black 24 x 24 grid in f64 takes 45 bodies: a restart, then the stop)
                assert 3 < want.iterations < 60 and want.cycles == 1 + want.iterations // 30 and want.breakdown == 0, (case.name, want.iterations)
                assert want.estimates[-1] < case.tol(dtype) <= min(want.estimates[:-1]), case.name
    # the level structure the GPU file relies on
    import trisolve_model as tm
    for g in (12, 24):
        off, col, _, _ = pc.grid(g, "red_black", F32)
        assert np.bincount(tm.levels(off, col, tm.LOWER)[0]).tolist() == [g * g // 2] * 2
        off, col, _, _ = pc.grid(g, "natural", F32)
        sizes = np.bincount(tm.levels(off, col, tm.LOWER)[0])
        assert len(sizes) == 2 * g - 1 and sizes.max() == g
        off, col, _, _ = pc.grid(g, "unsorted", F32)
        first = off[:-1].astype(np.int64)  # the diagonal leads every row and the west neighbour follows it: unsorted
        assert (col[first] == np.arange(g * g)).all() and (col[first[1:] + 1] < col[first[1:]]).any()


# ---- the binding ---------------------------------------------------------------------------------------------------------------
def test_binding_and_header_declare_both_entry_points():
    header = open(os.path.join(ROOT, "include", "sparsemat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    # (two arguments more than smh_gmres_solve*: precond and f)
    for name, n_args in (("smh_gmres_precond_solve", 15), ("smh_gmres_precond_solve_vec", 14)):
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    for k, name in enumerate(("NONE", "JACOBI", "SGS", "ILU")):
        assert re.search(r"#define\s+SMH_PRECOND_%s\s+%d\b" % (name, k), code) and getattr(_lib, "SMH_PRECOND_" + name) == k
    # decided before any device call: a NULL matrix, a kind out of range, a factor with another kind, ILU without one
    L = sm.lib()
    null, fake = None, 1  # (a non-NULL f is refused before it is looked at)
    for precond, f, text in ((_lib.SMH_PRECOND_JACOBI, null, b"NULL handle"), (4, null, b"precond"), (-1, null, b"precond"),
                             (_lib.SMH_PRECOND_SGS, fake, b"factor"), (_lib.SMH_PRECOND_NONE, fake, b"factor"),
                             (_lib.SMH_PRECOND_ILU, null, b"NULL handle")):
        assert L.smh_gmres_precond_solve(None, precond, f, None, 0, None, 0, 1e-10, 5, 30, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
        assert text in L.smh_last_error(), (precond, f, L.smh_last_error())
        assert L.smh_gmres_precond_solve_vec(None, precond, f, None, None, 1e-10, 5, 30, 0, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
        assert text in L.smh_last_error(), (precond, f, L.smh_last_error())
    s = sm.GMRES(1e-8, 50, precond="ilu")
    assert s.precond == "ilu" and s.factor is None and s.zero_pivot is None and sm.GMRES(1e-8, 50).precond is None
    with pytest.raises(ValueError):
        sm.GMRES(precond="ssor")
