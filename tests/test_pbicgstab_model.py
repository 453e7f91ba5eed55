"""CPU: tests/pbicgstab_model.py -- the contract of the right-preconditioned BiCGSTAB (smh_bicgstab_precond_solve*, bicgstab.hip).
With the identity it is bicgstab_model.bicgstab bit for bit; from x0 = 0 it is bicgstab_model.bicgstab on the product A o M^-1; on
the convection-diffusion grids the triangular preconditioners, and on badly scaled rows Jacobi, cut the bodies to a fraction; the
true residual of its x is the one the stop rule promises; every case of the GPU file moves a bit under each wrong variant of the
arithmetic it can tell apart; the binding and the header declare the two entry points."""
import math
import os
import re

import numpy as np
import pytest

import bicgstab_model as bm
import oracle
import pbicgstab_cases as pc
import pbicgstab_model as pb
import pgmres_model as pm
import sparsemat_amd as sm
from sparsemat_amd import _lib
from test_bicgstab_model import GRIDS
from test_gmres_model import true_residual
from test_pgmres_model import TABLE, TOLS, preconds, same, table_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
IDS = ["f32", "f64"]


def bits(r):
    return r.x.tobytes(), r.iterations, r.rr.tobytes(), r.breakdown


def scalars_equal(got, ref):
    """iterations, rr, the code and everything the stop tests saw"""
    return ((got.iterations, got.breakdown, got.converged, got.half_step) == (ref.iterations, ref.breakdown, ref.converged, ref.half_step)
            and same(got.rr, ref.rr) and same(np.array(got.ss_list), np.array(ref.ss_list)) and same(np.array(got.rr_list), np.array(ref.rr_list)))


# ---- 1: the identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_identity_is_bicgstab_bit_for_bit(dtype):
    """x, iterations, rr, the code, every s.s and every r.r: on test_bicgstab_model's convection-diffusion systems (to its
    tolerances, from x0 = 0 and from a random x0 with 7 bodies) and on bicgstab_model.EXACT."""
    tol = 1e-10 if dtype == F64 else 1e-4
    for g, c in GRIDS:
        off, col, val, b, _ = bm.convdiff_system(g, c, dtype)
        x1 = np.random.default_rng(100 + g).uniform(-1, 1, g * g).astype(dtype)
        for x0, t, iter_max in ((np.zeros(g * g, dtype), tol, 200), (x1, 0.0, 7)):
            want = bm.bicgstab(off, col, val, b, x0, t, iter_max)
            got = pb.pbicgstab(off, col, val, b, x0, t, iter_max, pm.identity)
            assert scalars_equal(got, want) and same(got.x, want.x), (g, c, iter_max)
            assert want.iterations == 7 or want.converged
    for name, a, b, iters, x, rr, breakdown, converged in bm.EXACT:
        off, col, val = bm.dense_to_crs(a, dtype)
        want = bm.bicgstab(off, col, val, np.array(b, dtype), np.zeros(len(b), dtype), 1e-6, 10)
        got = pb.pbicgstab(off, col, val, np.array(b, dtype), np.zeros(len(b), dtype), 1e-6, 10, pm.identity)
        assert scalars_equal(got, want) and same(got.x, want.x), name
        assert (got.iterations, got.x.tolist(), got.r_norm_squared, got.breakdown, got.converged) == (iters, x, rr, breakdown, converged), name


# ---- 2 - 4: the issue's table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("g,c", TABLE)
def test_table_bodies_and_true_residual(g, c, dtype):
    """test_pgmres_model.table_system's systems from x0 = 0 to tol: (2) iterations, rr, every s.s, every r.r and the code of every
    kind are bicgstab_model.bicgstab's on the product A o M^-1, bit for bit; (3) ILU(0) takes at most 0.35 and SGS at most 0.40 of
    the unpreconditioned bodies (the model's counts: none / Jacobi / SGS / ILU = 45 / 45 / 16 / 13 and 71 / 71 / 13 / 13 in f64,
    41 / 41 / 9 / 6 and 65 / 65 / 9 / 8 in f32: the largest ratios are 0.29 and 0.36); (4) the true residual of x, formed in f64,
    is below 2 tol (the largest ratio is 0.74)."""
    off, col, val, b = table_system(g, c, dtype)
    n, tol = g * g, TOLS[dtype]
    x0 = np.zeros(n, dtype)
    A = lambda v: oracle.spmv(off, col, val, v)
    plain = bm.bicgstab(off, col, val, b, x0, tol, 4000)
    assert plain.converged
    counts = {}
    for kind, M in preconds(off, col, val).items():
        got = pb.pbicgstab(off, col, val, b, x0, tol, 4000, M)
        ref = bm.bicgstab(off, col, val, b, x0, tol, 4000, product=lambda v: A(M(v)))
        assert scalars_equal(got, ref) and got.converged and got.breakdown == 0, kind
        true = true_residual(off, col, val, b, got.x)
        print(g, c, np.dtype(dtype).name, kind, got.iterations, "of", plain.iterations, "true/tol", true / tol)
        assert true < 2 * tol, (kind, true)
        counts[kind] = got.iterations
    assert counts["ilu"] <= 0.35 * plain.iterations, (counts, plain.iterations)
    assert counts["sgs"] <= 0.40 * plain.iterations, (counts, plain.iterations)
    assert counts["jacobi"] == plain.iterations  # (a constant diagonal: Jacobi changes nothing but a scale)
    want = {(24, F64): (45, 16, 13), (32, F64): (71, 13, 13), (24, F32): (41, 9, 6), (32, F32): (65, 9, 8)}[g, dtype]
    assert (plain.iterations, counts["sgs"], counts["ilu"]) == want  # (DESIGN.md's table)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_jacobi_on_scaled_rows(dtype):
    """convdiff2d(24, 1.0) with row i scaled by 2^k_i, k in -5 .. 5: Jacobi takes at most 0.15 of the unpreconditioned bodies (46 of
    456 in f64, 42 of 470 in f32), equals bicgstab_model.bicgstab on A o M^-1 bit for bit, and its true residual is below 2 tol.
    (The unpreconditioned f32 side ends at 2.3 tol: not asserted.)"""
    off, col, val, b = table_system(24, 1.0, dtype, scaled=True)
    tol, x0 = TOLS[dtype], np.zeros(576, dtype)
    M = pm.jacobi(off, col, val)
    A = lambda v: oracle.spmv(off, col, val, v)
    plain = bm.bicgstab(off, col, val, b, x0, tol, 6000)
    got = pb.pbicgstab(off, col, val, b, x0, tol, 6000, M)
    ref = bm.bicgstab(off, col, val, b, x0, tol, 6000, product=lambda v: A(M(v)))
    assert plain.converged and got.converged and scalars_equal(got, ref)
    true = true_residual(off, col, val, b, got.x)
    print(np.dtype(dtype).name, got.iterations, "of", plain.iterations, "true/tol", true / tol, "plain", true_residual(off, col, val, b, plain.x) / tol)
    assert got.iterations <= 0.15 * plain.iterations, (got.iterations, plain.iterations)
    assert true < 2 * tol, true
    assert (plain.iterations, got.iterations) == {F64: (456, 46), F32: (470, 42)}[dtype]  # (DESIGN.md's table)


# ---- 5: what the bit comparisons of the GPU file can tell apart --------------------------------------------------------------------
def can_tell(case, wrong, want):
    """Which wrong variants a case of the GPU file must move under.  Nothing shows on the exact and the all-NaN cases or without a
    body.  "reciprocal" and "fma" are Jacobi's alone (the other kinds apply no division of their own).  The sizes n <= 3 are there
    for the kernels' edge paths (sums of a handful of terms, a tiny system solved in n bodies)."""
    if case.exact or want.iterations == 0 or wrong in case.blind:
        return False
    if wrong in ("reciprocal", "fma") and case.kind != "jacobi":
        return False
    return case.n > 3


# per variant, a case that tells it (asserted below among all the others)
NAMED = {"left": "sgs convdiff2d(12, 1.0) natural, iter_max 5", "x unpreconditioned": "ilu convdiff2d(24, 1.0) red_black, to tol",
         "x one application": "sgs convdiff2d(24, 1.0) unsorted, to tol", "reciprocal": "jacobi n=259", "fma": "jacobi tol at a half step"}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", pc.KINDS)
def test_gpu_cases_move_under_every_wrong_variant(kind, dtype):
    moved = set()
    for case in [c for c in pc.BIT_CASES if c.kind == kind]:
        want = case.model(dtype)
        for wrong in pb.WRONG[1:]:
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
        for case in pc.J_SIZES:
            want = case.model(dtype)
            if case.n > 3:
                assert (want.iterations, want.breakdown, want.converged) == (8, 0, False), case.name
        zero = pc.J_SIZES[0].model(dtype)  # (an empty sum is zero: the first body's r^.v)
        assert (zero.iterations, zero.breakdown) == (1, 2)
        # the stops: the full step of body 10, the half step of body 11 -- neither on a batch boundary of 3 or 8
        full, half = (c.model(dtype) for c in pc.J_STOPS)
        tf, th = pc.J_STOPS[0].tol(dtype), pc.J_STOPS[1].tol(dtype)
        root = lambda v: math.sqrt(float(v))
        assert (full.iterations, full.half_step, full.converged, full.breakdown) == (10, False, True, 0)
        assert root(full.rr_list[-1]) < tf <= min(map(root, full.ss_list + full.rr_list[:-1]))
        assert (half.iterations, half.half_step, half.converged, half.breakdown) == (11, True, True, 0)
        assert root(half.ss_list[-1]) < th <= min(map(root, half.ss_list[:-1] + half.rr_list)) and len(half.rr_list) == 10
        inside, none = (c.model(dtype) for c in pc.J_ITER_MAX)
        assert (inside.iterations, inside.breakdown, inside.converged) == (11, 0, False)
        assert (none.iterations, none.breakdown) == (0, 0) and same(none.x, pc.J_ITER_MAX[1].system(dtype)[4]) and none.r_norm_squared > 0
        stop, b3, b1, b2, nan = (c.model(dtype) for c in pc.J_EXACT)
        assert (stop.iterations, stop.breakdown, stop.half_step, float(stop.rr)) == (1, 0, True, 0.0) and stop.x.tolist() == [0, 0, 0, 1.5, 0, 0, 0]
        assert (b3.iterations, b3.breakdown, float(b3.rr)) == (1, 3, 0.0) and b3.x.tolist() == [0, 0, 0, 1.5, 0, 0, 0]
        assert len(set(pc.J_EXACT[0].system(dtype)[2].tolist())) == 5
        assert (b1.iterations, b1.breakdown, float(b1.rr)) == (1, 1, 1.25) and b1.x.tolist() == [-0.5, 0.125]
        assert (b2.iterations, b2.breakdown, float(b2.rr)) == (1, 2, 0.0) and not b2.x.any()
        assert (nan.iterations, nan.breakdown) == (7, 0) and np.isnan(nan.x).all() and math.isnan(nan.r_norm_squared)
        halves = set()
        for case in pc.SGS + pc.ILU:
            want = case.model(dtype)
            if case.iter_max == 5:
                assert (want.iterations, want.breakdown, want.converged) == (5, 0, False), case.name
            else:
                assert 5 <= want.iterations <= 23 and want.breakdown == 0 and want.converged, (case.name, want.iterations)
                halves.add(want.half_step)
        assert halves == {True, False}  # both kinds of stop occur


# ---- 6, 7: the binding ---------------------------------------------------------------------------------------------------------
def test_binding_and_header_declare_both_entry_points():
    header = open(os.path.join(ROOT, "include", "sparsemat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    # two arguments more than smh_bicgstab_solve* (11 and 10): precond and f
    for name, n_args in (("smh_bicgstab_precond_solve", 13), ("smh_bicgstab_precond_solve_vec", 12)):
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name.replace("_precond", "")][1]) + 2
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert name in header.split("#define SMH_ABI_VERSION")[0], name  # (the list of additions)
    assert re.search(r"#define\s+SMH_ABI_VERSION\s+3\b", code)


def test_null_handles_and_bad_pairings_are_invalid_without_a_device():
    """decided before any device call: a NULL matrix, a kind out of range, a factor with another kind, ILU without one"""
    L = sm.lib()
    null, fake = None, 1  # (a non-NULL f is refused before it is looked at)
    for precond, f, text in ((_lib.SMH_PRECOND_JACOBI, null, b"NULL handle"), (4, null, b"precond"), (-1, null, b"precond"),
                             (_lib.SMH_PRECOND_SGS, fake, b"factor"), (_lib.SMH_PRECOND_NONE, fake, b"factor"),
                             (_lib.SMH_PRECOND_NONE, null, b"NULL handle"), (_lib.SMH_PRECOND_ILU, null, b"NULL handle")):
        assert L.smh_bicgstab_precond_solve(None, precond, f, None, 0, None, 0, 1e-10, 5, 0, None, None, None) == _lib.SMH_ERR_INVALID
        assert text in L.smh_last_error(), (precond, f, L.smh_last_error())
        assert L.smh_bicgstab_precond_solve_vec(None, precond, f, None, None, 1e-10, 5, 0, 0, None, None, None) == _lib.SMH_ERR_INVALID
        assert text in L.smh_last_error(), (precond, f, L.smh_last_error())
    s = sm.BiCGStab(1e-8, 50, precond="ilu")
    assert s.precond == "ilu" and s.factor is None and s.zero_pivot is None and sm.BiCGStab(1e-8, 50).precond is None
    with pytest.raises(ValueError):
        sm.BiCGStab(precond="ssor")
