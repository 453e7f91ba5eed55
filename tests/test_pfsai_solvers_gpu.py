"""GMRES and BiCGSTAB right-preconditioned by a pair of product handles (smh_gmres_fsai_solve*, smh_bicgstab_fsai_solve*) pinned BIT FOR
BIT to tests/pfsai_model.pgmres and tests/pbicgstab_model.pbicgstab in "device" mode: x, the number of entered bodies, f64(rr), the
cycles begun and the breakdown code -- f32 and f64, through both entry points, check_every 1, 3 and 8.  The models are fed by the
device's own checked products: the matrix's by `variant`, the pair's through AUTO for every application inside a body and through SEQ
for GMRES's cycle end -- which is how the tests tell that the cycle end's application is the gated storage-order one and that x is fed
from nothing else.  The pair is smh_crs_fsai_ns's (tests/test_fsai_ns_gpu.py pins its bits), or smh_crs_fsai's on a symmetric matrix.
(What no output can show is a cycle-end application that ran, dead, in a body that ends no cycle: it would write scratch that the
next body overwrites.  tools/pfsai_bench.py times that.)"""
import ctypes as C
import math

import numpy as np
import pytest

import bicgstab_model as bm
import fsai_cases as fc
import fsai_model as fm
import fsai_ns_cases as nc
import gmres_cases
import pbicgstab_model as pb
import pfsai_model as pf
import pgmres_model as pm
import sparsemat_amd as sm
import trisolve_model as tm
from kernel_forms import env
from sparsemat_amd import _lib
from test_bicgstab_gpu import assert_result as assert_bicgstab
from test_gmres_gpu import CHECK_EVERY, assert_result as assert_gmres, matrix, same, status_of
from test_pbicgstab_gpu import solve_host as bicgstab_host, solve_vec as bicgstab_vec
from test_pgmres_gpu import solve_host as gmres_host, solve_vec as gmres_vec
from test_solver_kernels_gpu import device_product

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
IDS = ["f32", "f64"]
SIZES = [1, 2, 3] + list(range(257, 265)) + [2049, 2051]


class System:
    """A system on the device: the handle, the pair (the device's own) and the checked products the models are fed with."""

    def __init__(self, off, col, val, b, x0, variant="seq", spd=False, model_pair=None):
        self.off, self.col, self.val, self.b, self.x0, self.variant = off, col, val, b, x0, variant
        self.a = matrix(off, col, val)
        g, gt, bad = self.a.fsai() if spd else self.a.fsai_ns()
        assert bad is None
        self.pair = (g, gt)
        gp, gtp = g.raw_parts(), gt.raw_parts()
        if model_pair is not None:  # (elsewhere the factor's bits are test_fsai_ns_gpu.py's business)
            assert all(np.array_equal(x, y) for x, y in zip(gp[:2] + gtp[:2], model_pair[0][:2] + model_pair[1][:2]))
            assert same(gp[2], model_pair[0][2]) and same(gtp[2], model_pair[1][2]), "the device's pair is not the model's"
        self.product = device_product(self.a, variant, off, col, val)
        first, second = device_product(g, "auto", *gp), device_product(gt, "auto", *gtp)
        self.body = lambda v: second(first(v))
        first_seq, second_seq = device_product(g, "seq", *gp), device_product(gt, "seq", *gtp)
        self.end = lambda v: second_seq(first_seq(v))

    def gmres_model(self, tol, iter_max, restart, end=None):
        return pf.pgmres(self.off, self.col, self.val, self.b, self.x0, tol, iter_max, restart, self.body, precond_end=end or self.end, product=self.product)

    def bicgstab_model(self, tol, iter_max):
        return pb.pbicgstab(self.off, self.col, self.val, self.b, self.x0, tol, iter_max, self.body, product=self.product)

    def check_gmres(self, tol, iter_max, restart, check_every=CHECK_EVERY, what=""):
        want = self.gmres_model(tol, iter_max, restart)
        assert_gmres(gmres_host(self.a, "fsai", self.b, self.x0, tol, iter_max, restart, self.variant, self.pair), want, (what, "host"))
        for ce in check_every:
            assert_gmres(gmres_vec(self.a, "fsai", self.b, self.x0, tol, iter_max, restart, ce, self.variant, self.pair), want, (what, "vec/%d" % ce))
        return want

    def check_bicgstab(self, tol, iter_max, check_every=CHECK_EVERY, what=""):
        want = self.bicgstab_model(tol, iter_max)
        assert_bicgstab(bicgstab_host(self.a, "fsai", self.b, self.x0, tol, iter_max, self.variant, self.pair), want, (what, "host"))
        for ce in check_every:
            assert_bicgstab(bicgstab_vec(self.a, "fsai", self.b, self.x0, tol, iter_max, ce, self.variant, self.pair), want, (what, "vec/%d" % ce))
        return want


def tridiag(n, dtype, variant="seq"):
    return System(*gmres_cases.ns(n, dtype), variant=variant)


def grid(g, dtype, variant="seq", zero_x0=False):
    """convdiff2d(g, 1.0), rows sorted, with the model's pair asserted; b and x0 uniform (zero_x0: x0 = 0)"""
    name = "convdiff%d" % g
    off, col, val = nc.matrix(name, dtype)
    b, x0 = gmres_cases.rhs(g * g, dtype, g)
    return System(off, col, val, b, np.zeros_like(x0) if zero_x0 else x0, variant=variant, model_pair=nc.factor(name, dtype)[:2])


def banded(dtype, variant="seq"):
    """300 rows with 16 columns on either side of the diagonal, values of their own: the factors' rows hold up to 17 entries, so their
    AUTO product is the lane-group kernel, whose sums are not in storage order -- its bits part from SEQ's."""
    n = 300
    off, col, val = nc.from_patterns([np.arange(max(0, i - 16), i) for i in range(n)], [np.arange(i + 1, min(n, i + 17)) for i in range(n)], dtype, seed=11)
    b, x0 = gmres_cases.rhs(n, dtype, 3)
    s = System(off, col, val, b, x0, variant=variant)
    assert s.pair[0].resolved_variant()[0] == s.pair[1].resolved_variant()[0] == "vector"
    return s


def tol_of(dtype):
    return 1e-4 if dtype == F32 else 1e-8


# ---- the path sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", SIZES)
def test_gmres_bits_at_every_path_size(gpu, dtype, n):
    """tridiag_ns of n = 1, 2, 3; 257 .. 264 (every n mod 16 bytes, one workgroup); 2049 / 2051 (nine workgroups).  GMRES(3), 8 bodies
    from a non-zero x0: three cycles, the last cut short by iter_max (n <= 3: the Krylov space is exhausted first)."""
    want = tridiag(n, dtype).check_gmres(0.0, 8, 3, what=n)
    if n > 3:
        assert (want.iterations, want.cycles, want.breakdown) == (8, 3, 0)
    else:
        assert want.iterations <= 8 and want.cycles >= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", SIZES)
def test_bicgstab_bits_at_every_path_size(gpu, dtype, n):
    """The same sizes, 6 bodies from a non-zero x0 (n <= 3: a breakdown or the exact solution ends it sooner)."""
    want = tridiag(n, dtype).check_bicgstab(0.0, 6, what=n)
    if n > 3:
        assert want.iterations == 6 and want.breakdown == 0


# ---- restarts, stops, iter_max --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("g, restart", [(12, 1), (12, 5), (24, 30)])
def test_gmres_restart_lengths_with_three_cycles(gpu, dtype, g, restart):
    """convdiff2d(12, 1.0) with GMRES(1) and GMRES(5), convdiff2d(24, 1.0) with GMRES(30): 2 m + 2 bodies from a random x0 -- two full
    cycles and a third begun (GMRES(1): four), every cycle end through the gated products."""
    s = grid(g, dtype)
    want = s.check_gmres(0.0, 2 * restart + 2, restart, check_every=(3, 8), what=(g, restart))
    cycles = -(-(2 * restart + 2) // restart)  # (GMRES(1): every body is a cycle)
    assert want.iterations == 2 * restart + 2 and want.cycles == cycles >= 3 and want.breakdown == 0 and len(want.ends) == cycles


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gmres_stop_on_tol_inside_a_batch_and_on_its_boundary(gpu, dtype):
    """convdiff2d(24, 1.0) from x0 = 0, GMRES(30) to tol: the estimate falls under tol in body k, inside a replayed batch for
    check_every 1, 3 and 8 and on a batch boundary for check_every = k; the stopping body's x update is visible and x solves the
    system.  Fewer than half of plain GMRES(30)'s bodies on the device too."""
    s = grid(24, dtype, zero_x0=True)
    tol = tol_of(dtype)
    want = s.check_gmres(tol, 500, 30, what="stop")
    k = want.iterations
    assert 8 < k < 100 and (k % 8 or k % 3) and want.breakdown == 0 and want.estimates[-1] < tol <= min(want.estimates[:-1])
    assert not same(want.x, s.gmres_model(0.0, k - 1, 30).x)
    assert_gmres(gmres_vec(s.a, "fsai", s.b, s.x0, tol, 500, 30, k, "seq", s.pair), want, "a batch boundary")
    r = s.b.astype(np.longdouble) - s.product(want.x).astype(np.longdouble)
    assert float(np.sqrt(np.sum(r * r))) < 2 * tol
    plain = sm.GMRES(tol, 2000, 30, variant="seq")
    plain.solve(s.a, s.b, s.x0.copy())
    assert k <= 0.5 * plain.iterations, (k, plain.iterations)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gmres_iter_max_inside_a_cycle_and_at_a_cycle_end(gpu, dtype):
    """tol = 0 on convdiff2d(12, 1.0), GMRES(5): iter_max 12 (inside the third cycle, inside a batch of 3 and of 8), 10 (at the end of
    the second cycle: a stop, no third cycle begins) and 0 (no body: x0 comes back, the initial r.r is reported)."""
    s = grid(12, dtype)
    for iter_max, cycles in ((12, 3), (10, 2), (0, 1)):
        want = s.check_gmres(0.0, iter_max, 5, what=iter_max)
        assert (want.iterations, want.cycles, want.breakdown) == (iter_max, cycles, 0)
    assert same(want.x, s.x0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bicgstab_stops_and_iter_max(gpu, dtype):
    """convdiff2d(24, 1.0) from x0 = 0 to tol (the stop inside a batch, and with check_every = k on its boundary; at most 0.65 of
    plain BiCGSTAB's bodies), then tol = 0 with iter_max 11 (inside a batch of 3 and of 8) and 0."""
    s = grid(24, dtype, zero_x0=True)
    tol = tol_of(dtype)
    want = s.check_bicgstab(tol, 500, what="stop")
    k = want.iterations
    assert 5 < k < 100 and want.converged and want.breakdown == 0
    assert_bicgstab(bicgstab_vec(s.a, "fsai", s.b, s.x0, tol, 500, k, "seq", s.pair), want, "a batch boundary")
    r = s.b.astype(np.longdouble) - s.product(want.x).astype(np.longdouble)
    assert float(np.sqrt(np.sum(r * r))) < 2 * tol
    plain = sm.BiCGStab(tol, 2000, variant="seq")
    plain.solve(s.a, s.b, s.x0.copy())
    assert k <= 0.65 * plain.iterations, (k, plain.iterations)
    s = grid(12, dtype)
    for iter_max in (11, 0):
        want = s.check_bicgstab(0.0, iter_max, what=iter_max)
        assert want.iterations == iter_max and want.breakdown == 0
    assert same(want.x, s.x0)


# ---- the cycle end's application -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cycle_end_is_formed_by_the_gated_products_and_nothing_else_feeds_x(gpu, dtype):
    """A banded system whose factors' own product is the lane-group kernel, GMRES(5), 12 bodies: two or three cycle ends.  On these factors
    the storage-order product and the handles' own differ in bits, so a model that forms q through AUTO parts from the right one in x
    and in nothing else -- and the device equals the right one.  (On the grids both products are K1s's, bit for bit SEQ's.)"""
    s = banded(dtype)
    want = s.gmres_model(0.0, 12, 5)
    got = gmres_vec(s.a, "fsai", s.b, s.x0, 0.0, 12, 5, 8, "seq", s.pair)
    assert_gmres(got, want, "the gated cycle end")
    # (what lets the test tell; in f32 the third cycle may begin on a residual that is exactly zero: breakdown 2, two cycle ends)
    assert len(want.ends) >= 2 and all(not same(s.end(t), s.body(t)) for t in want.ends)
    through_auto = s.gmres_model(0.0, 12, 5, end=s.body)
    assert not same(through_auto.x, want.x) and (through_auto.iterations, through_auto.cycles, through_auto.rr) == (want.iterations, want.cycles, want.rr)
    assert not same(got[0], through_auto.x)
    # x moves at a cycle end alone: after 4 bodies (no cycle has ended, then iter_max ends it) x = x0 + q of that one end
    early = s.gmres_model(0.0, 4, 5)
    assert len(early.ends) == 1
    assert_gmres(gmres_host(s.a, "fsai", s.b, s.x0, 0.0, 4, 5, "seq", s.pair), early, "one cycle end")
    with np.errstate(all="ignore"):
        assert same(early.x, s.x0 + s.end(early.ends[0]))


# ---- the products of A, the node budget, the SPD pair ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stream_seq_and_auto_products_of_the_matrix(gpu, dtype):
    """tridiag_ns(259): GMRES(4) with 11 bodies and BiCGSTAB with 7, from a random x0, through the three products of A; the model takes
    each from the device.  The pair's own products are AUTO and SEQ whatever `variant` says."""
    for variant in ("stream", "seq", "auto"):
        s = tridiag(259, dtype, variant)
        want = s.check_gmres(0.0, 11, 4, check_every=(3,), what=variant)
        assert (want.iterations, want.cycles, want.breakdown) == (11, 3, 0)
        want = s.check_bicgstab(0.0, 7, check_every=(3,), what=variant)
        assert want.iterations == 7


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_node_budget_changes_no_bit(gpu, dtype):
    """A body holds three (GMRES) or four (BiCGSTAB) applications' worth of product nodes.  With the budget of a captured batch lowered
    to 100 nodes (SMH_SGS_GRAPH_NODES) batches of 8 bodies become smaller; lowered to 8 a single body is beyond it and the loop runs
    uncaptured.  Both give the bits of the replayed route, on iter_max and on a stop on tol."""
    s = grid(12, dtype, zero_x0=True)
    tol = tol_of(dtype)
    for model, host, vec, check in ((s.gmres_model(0.0, 12, 5), lambda: gmres_host(s.a, "fsai", s.b, s.x0, 0.0, 12, 5, "seq", s.pair),
                                     lambda: gmres_vec(s.a, "fsai", s.b, s.x0, 0.0, 12, 5, 8, "seq", s.pair), assert_gmres),
                                    (s.gmres_model(tol, 500, 30), lambda: gmres_host(s.a, "fsai", s.b, s.x0, tol, 500, 30, "seq", s.pair),
                                     lambda: gmres_vec(s.a, "fsai", s.b, s.x0, tol, 500, 30, 8, "seq", s.pair), assert_gmres),
                                    (s.bicgstab_model(0.0, 11), lambda: bicgstab_host(s.a, "fsai", s.b, s.x0, 0.0, 11, "seq", s.pair),
                                     lambda: bicgstab_vec(s.a, "fsai", s.b, s.x0, 0.0, 11, 8, "seq", s.pair), assert_bicgstab),
                                    (s.bicgstab_model(tol, 500), lambda: bicgstab_host(s.a, "fsai", s.b, s.x0, tol, 500, "seq", s.pair),
                                     lambda: bicgstab_vec(s.a, "fsai", s.b, s.x0, tol, 500, 8, "seq", s.pair), assert_bicgstab)):
        replays = []
        for nodes in (None, "100", "8"):
            with env(SMH_SGS_GRAPH_NODES=nodes):
                check(vec(), model, ("budget", nodes))
                replays.append(sm.lib().smh_last_solve_replays())
                check(host(), model, ("budget, host", nodes))
        assert replays[2] == 0, replays  # (the capture was dropped)
        assert replays[0] > 0 and replays[1] >= replays[0], replays


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_spd_pair_on_a_symmetric_matrix(gpu, dtype):
    """(G, G^T) of smh_crs_fsai on the suite's SPD table row 1: M^-1 = G^T G through the same entry points."""
    off, col, val = fc.matrix("table1", dtype)
    n = len(off) - 1
    b, x0 = gmres_cases.rhs(n, dtype, 5)
    goff, gcol, gval, bad = fc.factor("table1", dtype)
    s = System(off, col, val, b, x0, spd=True, model_pair=((goff, gcol, gval), fm.transpose(goff, gcol, gval)))
    want = s.check_gmres(0.0, 12, 5, check_every=(3, 8), what="spd")
    assert (want.iterations, want.cycles) == (12, 3)
    want = s.check_bicgstab(0.0, 7, check_every=(3, 8), what="spd")
    assert want.iterations == 7


# ---- the Python classes, reproducibility, the statuses --------------------------------------------------------------------------
def test_python_classes_factor_by_themselves(gpu):
    """precond="fsai" with factor=None calls mat.fsai_ns(): the bits of a passed pair; `factor` and `singular` are left behind."""
    s = grid(12, F64)
    gl, gu, _ = nc.factor("convdiff12", F64)
    want = s.gmres_model(0.0, 12, 5)
    own = sm.GMRES(0.0, 12, 5, variant="seq", precond="fsai")
    x = s.x0.copy()
    own.solve(s.a, s.b, x)
    assert_gmres((x, own.iterations, own.r_norm_squared, own.cycles, own.breakdown), want, "factor=None")
    assert own.singular is None and same(own.factor[0].raw_parts()[2], gl[2]) and same(own.factor[1].raw_parts()[2], gu[2])
    own.solve(s.a, s.b, s.x0.copy(), factor=s.pair)
    assert own.factor is s.pair and own.singular is None and own.iterations == want.iterations
    want = s.bicgstab_model(0.0, 7)
    own = sm.BiCGStab(0.0, 7, variant="seq", precond="fsai")
    x = s.x0.copy()
    own.solve(s.a, s.b, x)
    assert_bicgstab((x, own.iterations, own.r_norm_squared, own.breakdown, own.converged), want, "factor=None")
    assert own.singular is None and same(own.factor[0].raw_parts()[2], gl[2])
    # a singular matrix: the row is reported and the solve runs on IEEE's values (NaN in, NaN out, no error)
    sing = matrix(*tm.from_rows([[(0, 1.0), (1, 2.0)], [(0, 2.0), (1, 4.0)]], F64))
    x = np.zeros(2)
    own.solve(sing, np.ones(2), x)
    assert own.singular == 1 and np.isnan(x).all()


def test_solves_are_reproducible(gpu):
    s = grid(24, F32)
    first = gmres_vec(s.a, "fsai", s.b, s.x0, 1e-4, 200, 10, 3, "auto", s.pair)
    for ce in (3, 8, 1):
        again = gmres_vec(s.a, "fsai", s.b, s.x0, 1e-4, 200, 10, ce, "auto", s.pair)
        assert same(again[0], first[0]) and again[1:] == first[1:]
    first = bicgstab_vec(s.a, "fsai", s.b, s.x0, 1e-4, 200, 3, "auto", s.pair)
    for ce in (3, 8, 1):
        again = bicgstab_vec(s.a, "fsai", s.b, s.x0, 1e-4, 200, ce, "auto", s.pair)
        assert same(again[0], first[0]) and again[1:] == first[1:]


def test_statuses_leave_x_untouched(gpu):
    f = F64
    L = sm.lib()
    off, col, val = nc.matrix("convdiff12", f)
    n = 144
    a = matrix(off, col, val)
    gl, gu, _ = a.fsai_ns()
    b, x = np.ones(n, f), np.full(n, 7.0)
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x)
    solvers = [lambda: sm.GMRES(1e-10, 50, variant="seq", precond="fsai"), lambda: sm.BiCGStab(1e-10, 50, variant="seq", precond="fsai")]
    small = matrix(*nc.matrix("tridiag3000", f)).fsai_ns()
    g32 = matrix(*[p if i < 2 else p.astype(F32) for i, p in enumerate(gl.raw_parts())])
    rect = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 1], np.ones(2, f))
    orphan = sm.SparseMatCRS.from_triplets([1, 0, 1, 0], [1, 0, 0, 1], np.ones(4, f), into_crs=True)
    two = matrix([0, 2, 4], [0, 1, 0, 1], np.array([4.0, 1, 1, 4]))
    gp = gl.raw_parts()
    beyond = sm.SparseMatCRS.from_raw_parts(n, n, gp[0], np.where(np.arange(len(gp[1])) == 5, n + 3, gp[1]).astype(np.uint32), gp[2], validate=False)
    assert orphan.orphans() == 1
    for make in solvers:
        s = make()
        pair = (gl, gu)
        # the pair's: smh_pcg_fsai_solve's
        for factor, status in (((small[0], gu), _lib.SMH_ERR_DIM_MISMATCH), ((gl, small[1]), _lib.SMH_ERR_DIM_MISMATCH), ((g32, gu), _lib.SMH_ERR_INVALID),
                               ((gl, g32), _lib.SMH_ERR_INVALID), ((rect, gu), _lib.SMH_ERR_NOT_SQUARE), ((gl, rect), _lib.SMH_ERR_NOT_SQUARE),
                               ((beyond, gu), _lib.SMH_ERR_INDEX_RANGE), ((gl, beyond), _lib.SMH_ERR_INDEX_RANGE)):
            assert status_of(lambda: s.solve(a, b, x, factor=factor))[0] == status
            assert status_of(lambda: s.solve(a, bd, xd, factor=factor))[0] == status
        st, msg = status_of(lambda: s.solve(two, np.ones(2), np.full(2, 7.0), factor=(orphan, two)))
        assert st == _lib.SMH_ERR_INVALID and "orphan" in msg and "FSAI" in msg
        st, msg = status_of(lambda: s.solve(two, np.ones(2), np.full(2, 7.0), factor=(two, orphan)))
        assert st == _lib.SMH_ERR_INVALID and "orphan" in msg
        # the solver's own: not square, the lengths, b and x the same storage, a DenseVec of the other dtype
        assert status_of(lambda: s.solve(rect, np.ones(2, f), np.full(2, 7.0), factor=pair))[0] == _lib.SMH_ERR_NOT_SQUARE
        assert status_of(lambda: s.solve(a, np.ones(n - 1, f), x, factor=pair))[0] == _lib.SMH_ERR_DIM_MISMATCH
        assert status_of(lambda: s.solve(a, b, np.full(n - 1, 7.0), factor=pair))[0] == _lib.SMH_ERR_DIM_MISMATCH
        assert status_of(lambda: s.solve(a, sm.DenseVec.from_vec(np.ones(n + 1, f)), xd, factor=pair))[0] == _lib.SMH_ERR_DIM_MISMATCH
        assert status_of(lambda: s.solve(a, xd, xd, factor=pair))[0] == _lib.SMH_ERR_INVALID
        assert status_of(lambda: s.solve(a, x, x, factor=pair))[0] == _lib.SMH_ERR_INVALID
        assert status_of(lambda: s.solve(a, sm.DenseVec.from_vec(np.ones(n, F32)), xd, factor=pair))[0] == _lib.SMH_ERR_INVALID
        assert s.iterations is None  # (a refused call reports nothing)
    for fb, fx in ((b, x), (bd, xd)):
        st, msg = status_of(lambda: sm.GMRES(1e-10, 50, restart=129, variant="seq", precond="fsai").solve(a, fb, fx, factor=(gl, gu)))
        assert st == _lib.SMH_ERR_INVALID and "restart" in msg
    # NULL handles and vectors of the raw entry points
    gm_host = lambda *h: L.smh_gmres_fsai_solve(*h, b.ctypes.data, n, x.ctypes.data, n, 1e-10, 5, 30, 0, None, None, None, None)
    bi_host = lambda *h: L.smh_bicgstab_fsai_solve(*h, b.ctypes.data, n, x.ctypes.data, n, 1e-10, 5, 0, None, None, None)
    gm_vec = lambda *h: L.smh_gmres_fsai_solve_vec(*h, 1e-10, 5, 30, 0, 0, None, None, None, None)
    bi_vec = lambda *h: L.smh_bicgstab_fsai_solve_vec(*h, 1e-10, 5, 0, 0, None, None, None)
    for host, vec in ((gm_host, gm_vec), (bi_host, bi_vec)):
        assert host(None, gl._h, gu._h) == host(a._h, None, gu._h) == host(a._h, gl._h, None) == _lib.SMH_ERR_INVALID
        assert vec(None, gl._h, gu._h, bd._h, xd._h) == vec(a._h, None, gu._h, bd._h, xd._h) == vec(a._h, gl._h, None, bd._h, xd._h) == _lib.SMH_ERR_INVALID
        assert vec(a._h, gl._h, gu._h, None, xd._h) == vec(a._h, gl._h, gu._h, bd._h, bd._h) == _lib.SMH_ERR_INVALID
    assert L.smh_gmres_fsai_solve(a._h, gl._h, gu._h, None, n, x.ctypes.data, n, 1e-10, 5, 30, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_bicgstab_fsai_solve(a._h, gl._h, gu._h, None, n, x.ctypes.data, n, 1e-10, 5, 0, None, None, None) == _lib.SMH_ERR_INVALID
    assert x.tolist() == [7.0] * n and xd.to_numpy().tolist() == [7.0] * n
    # the existing entry points keep their refusals: code 4 is no kind, and a pair's handle is no ILU factor's business of another kind
    assert L.smh_gmres_precond_solve_vec(a._h, 4, None, bd._h, xd._h, 1e-10, 5, 30, 0, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_bicgstab_precond_solve_vec(a._h, _lib.SMH_PRECOND_SGS, gl._h, bd._h, xd._h, 1e-10, 5, 0, 0, None, None, None) == _lib.SMH_ERR_INVALID
    # ... and the output pointers may be NULL; restart 0 is GMRES(30)
    assert L.smh_gmres_fsai_solve_vec(a._h, gl._h, gu._h, bd._h, xd._h, 1e-10, 50, 0, _lib.VARIANTS["seq"], 0, None, None, None, None) == 0
    sys = System(off, col, val, b, x)
    assert same(xd.to_numpy(), sys.gmres_model(1e-10, 50, 30).x)
    xd = sm.DenseVec.from_vec(x)
    assert L.smh_bicgstab_fsai_solve_vec(a._h, gl._h, gu._h, bd._h, xd._h, 1e-10, 50, _lib.VARIANTS["seq"], 0, None, None, None) == 0
    assert same(xd.to_numpy(), sys.bicgstab_model(1e-10, 50).x)
