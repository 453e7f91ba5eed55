"""tests/par_cg_model.py pinned without a GPU: with one block it is cg_model.cg bit for bit, in "sequential" mode it is the
oracle, its "device" sums stay within the bound their own depth gives against exact sums -- and every case of
tests/test_par_cg_bits_gpu.py (tests/par_cg_cases.py) moves a bit of what the device reports under each mistake that can touch
it, so that equal bits on the device mean the right order and nothing else."""
import math

import numpy as np
import pytest

import cg_model
import oracle
import par_cg_cases as pc
import par_cg_model as pm
from par_cg_cases import same

DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
SMALL = [1, 2, 3, 5, 255, 257]  # (tests/test_cg_bits_gpu.py)


def system(n, dtype, seed, x0_random):
    return cg_model.tridiag(n, dtype, seed=seed) + pc.rhs(n, dtype, seed, x0_random)


def assert_same_result(got, want, what):
    assert got.iterations == want.iterations, what
    for name in ("x", "r", "p", "rr0"):
        assert same(getattr(got, name), getattr(want, name)), (what, name)
    assert same(np.array(got.rr_list), np.array(want.rr_list)), (what, "rr_list")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_block_is_the_single_matrix_solver(dtype):
    """cuts = [0, n]: the lone block still sends each of its three values through a fold of ONE value, and its fused partials
    through launch_fold2's two stages where the single-matrix solver folds up to 1024 of them with one workgroup.  Every one of
    these sums starts at +0 and adds the value (to +0s only), which returns the value's own bits unless it is -0; r.r and p.Ap
    are sums that began at +0 themselves and are never -0.  So NOTHING differs, not even the sign of a zero: x, r, p, every r.r
    and the body count are compared without exception.  (reduce_blocks(tiles) stays 1 up to 2048 tiles, and beyond 1024 the
    single-matrix solver takes the same two stages: 262 144 + 259 and 524 288 + 1027 rows are 1026 and 2053 tiles.)"""
    for k, n in enumerate(SMALL + [2051, 2049]):
        off, col, val, b, x0 = system(n, dtype, n % 97, bool(k % 2))
        for tol, it in ((0.0, 6), (1e-3, 50)):
            assert_same_result(pm.par_cg(off, col, val, b, x0, tol, it, [0, n]), cg_model.cg(off, col, val, b, x0, tol, it), ("separate", n, tol))
    for k, n in enumerate([255, 257, 2051, 262_144 + 259, 524_288 + 1027]):
        off, col, val, b, x0 = system(n, dtype, n % 97, bool(k % 2))
        it = 6 if n < 100_000 else 2
        assert_same_result(pm.par_cg(off, col, val, b, x0, 0.0, it, [0, n], fused=True), cg_model.cg(off, col, val, b, x0, 0.0, it, fused=True), ("fused", n))
    z = np.zeros(37, dtype)  # b = 0: the reference's 0 / 0
    off, col, val = cg_model.tridiag(37, dtype, seed=1)
    assert_same_result(pm.par_cg(off, col, val, z, z, 1e-6, 5, [0, 37]), cg_model.cg(off, col, val, z, z, 1e-6, 5), "b = 0")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cuts", [[0, 259], [0, 1, 259], [0, 100, 100, 259], pc.EMPTY_CUTS[:2] + [259], [0, 3, 7, 64, 65, 258, 259]], ids=lambda c: "%d-blocks" % (len(c) - 1))
def test_sequential_and_wide_modes_know_no_blocks(cuts, dtype):
    """ "sequential" is the oracle bit for bit whatever the cuts, "wide" is cg_model.cg's."""
    n = 259
    off, col, val, b, x0 = system(n, dtype, 4, True)
    for tol, iter_max in ((0.0, 9), (1e-3, 50), (0.0, 0)):
        got = pm.par_cg(off, col, val, b, x0, tol, iter_max, cuts, mode="sequential")
        o_x, o_iters, o_rr = oracle.cg(n, n, off, col, val, b, x0, tol=tol, iter_max=iter_max)
        assert got.iterations == o_iters and same(got.x, o_x) and same(np.float64(got.r_norm_squared), np.float64(o_rr)), (tol, iter_max)
        assert_same_result(pm.par_cg(off, col, val, b, x0, tol, iter_max, cuts, mode="wide"), cg_model.cg(off, col, val, b, x0, tol, iter_max, mode="wide"), "wide")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cuts", [pc.SPLIT7, pc.SPLIT7_REV, pc.EVEN_CUTS, pc.EMPTY_CUTS, [0, 300_003]], ids=["split7", "split7-rev", "even3", "empty", "one-large"])
def test_block_sums_sum_their_terms(cuts, dtype):
    """The three sums of a body in "device" mode against math.fsum of the same (already rounded) terms, within
    depth * eps * sum|t_i| -- test_cg_model.py's bound, the depth now par_cg_model.tree_depth: the block's own tree and the
    cross-block fold -- and against "wide"; a term of its own magnitude is lost in no block, whichever way its dot goes."""
    n = cuts[-1]
    rng = np.random.default_rng(n)
    x, y = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
    eps = float(np.finfo(dtype).eps)
    for fused in (False, True):
        sums = pm.BlockSums(cuts, dtype, fused)
        for kind, got, u, v in (("rr0", sums.rr0(x), x, x), ("rr", sums.rr(x), x, x), ("pap_fused" if fused else "pap", sums.pap(x, y), x, y)):
            terms = u * v
            exact = math.fsum(terms.astype(np.float64).tolist())
            scale = math.fsum(np.abs(terms).astype(np.float64).tolist())
            assert got.dtype == np.dtype(dtype)
            assert abs(float(got) - exact) <= pm.tree_depth(kind, cuts, dtype) * eps * scale, (kind, fused)
            assert abs(float(got) - float(cg_model.wide_dot(u, v))) <= (pm.tree_depth(kind, cuts, dtype) + 1) * eps * scale, (kind, fused)
        for pos in sorted(set([0, n - 1] + [c for c in cuts[1:-1] if c < n] + [c - 1 for c in cuts[1:] if c > 0])):
            t, one = np.zeros(n, dtype), np.ones(n, dtype)
            t[pos] = 3.0
            assert sums.pap(t, one) == 3.0 and sums.rr0(np.sqrt(t)) == dtype(np.sqrt(dtype(3.0))) ** 2 and sums.rr(np.sqrt(t)) == sums.rr0(np.sqrt(t)), pos


CASES = [pytest.param(name, build, id="%s-%s" % (name, IDS[DTYPES.index(dt)])) for dt in DTYPES for name, build in pc.builders(dt)]


@pytest.mark.parametrize("name,build", CASES)
def test_gpu_cases_tell_right_from_wrong(name, build):
    """Every case of tests/test_par_cg_bits_gpu.py under every mistake of par_cg_model.WRONG: where the mistake can touch the
    case at all (par_cg_cases.applicable says when, and why not otherwise) at least one bit of x, of some body's r.r or the body
    count moves within the bodies the case runs; where it cannot, nothing moves.  The seeds in par_cg_cases.SEEDS are the
    smallest, counted from 0, at which this holds.  The stop test placed after beta ("late_stop") can move no reported bit in any
    case -- x and r.r of the stopping body are complete before either placement -- so it is shown on p, and its observable
    sibling ("stop_next": the loop leaves one body late) on the cases that stop on tol."""
    case = build()
    assert case.name == name
    right = case.model()
    assert np.isfinite(right.x).all() and right.iterations == (pc.STOP_BODY if case.tol > 0 else case.iter_max)
    for wrong in pm.WRONG:
        got = case.model(wrong=(wrong,))
        assert pc.differs(got, right) == pc.applicable(case, wrong), (case.name, wrong)
    if case.tol > 0:
        late = case.model(wrong=("late_stop",))
        assert not same(late.p, right.p) and same(late.x, right.x) and same(late.r, right.r)
        assert case.model(wrong=("stop_next",)).iterations == pc.STOP_BODY + 1
        assert not same(right.x, case.model(tol=0.0, iter_max=pc.STOP_BODY - 1).x)  # (the stopping body's x update is visible in x)


def test_breakdown_case_has_no_bits_to_move():
    """b = 0, x0 = 0: every reported number is NaN or the initial r.r = +0, whatever the order: this case of the GPU file
    checks the body count and the NaN pattern, not the order."""
    n = pc.N7
    off, col, val = cg_model.tridiag(n, np.float32, seed=3)
    z = np.zeros(n, np.float32)
    got = pm.par_cg(off, col, val, z, z, 1e-6, 5, pc.SPLIT7)
    o_x, o_it, o_rr = oracle.cg(n, n, off, col, val, z, z, tol=1e-6, iter_max=5)
    assert got.iterations == o_it == 5 and np.isnan(got.x).all() and np.isnan(o_x).all() and np.isnan(got.r_norm_squared) and np.isnan(o_rr)
