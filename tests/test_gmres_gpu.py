"""The device-resident restarted GMRES (gmres.hip) pinned BIT FOR BIT to tests/gmres_model.py's "device" mode: x, the number of
entered bodies, the number of cycles begun, f64(rr) and the breakdown code -- f32 and f64, through both entry points, at the sizes
where each path of the sweeps is first entered, at restart lengths around the dots' column tile, stopping inside a cycle, exactly
at j = m, on and inside a replayed batch, on iter_max inside a cycle, inside a batch and at a cycle end, on both breakdown codes,
from a non-zero x0, on NaN data, through the STREAM, SEQ and AUTO products and a few kernel families of tests/kernel_forms.py.
The cases live in tests/gmres_cases.py; tests/test_gmres_model.py shows without a GPU that each of them moves a bit under every
wrong variant of the arithmetic it can tell apart.

The model (not this file) says what the arithmetic is; tests/test_gmres_model.py pins the model without a GPU."""
import math

import numpy as np
import pytest

import bicgstab_model as bm
import gmres_cases
import gmres_model as gm
import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
CHECK_EVERY = (1, 3, 8)


def same(a, b):
    """bit equality (any NaN equals any NaN: its sign and payload are not arithmetic)"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def assert_result(got, want, what):
    """got: (x, iterations, r_norm_squared, cycles, breakdown) of the device; want: a gmres_model.Result"""
    x, iters, rr, cycles, breakdown = got
    assert iters == want.iterations, (what, "iterations", iters, want.iterations)
    assert cycles == want.cycles, (what, "cycles", cycles, want.cycles)
    assert breakdown == want.breakdown, (what, "breakdown", breakdown, want.breakdown)
    assert same(np.float64(rr), np.float64(want.r_norm_squared)), (what, "r.r", rr, want.r_norm_squared)
    bad = np.flatnonzero(~((x == want.x) | (np.isnan(x) & np.isnan(want.x))))
    assert same(x, want.x), (what, "x", len(bad), bad[:5], x[bad[:5]], want.x[bad[:5]])


def matrix(off, col, val):
    n = len(off) - 1
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)


def results(s, x):
    return x, s.iterations, s.r_norm_squared, s.cycles, s.breakdown


def solve_host(a, b, x0, tol, iter_max, restart, variant="seq"):
    """smh_gmres_solve: numpy arrays (check_every is the driver's default, 8)"""
    x = x0.copy()
    s = sm.GMRES(tol, iter_max, restart, variant=variant)
    s.solve(a, b, x)
    return results(s, x)


def solve_vec(a, b, x0, tol, iter_max, restart, check_every, variant="seq"):
    """smh_gmres_solve_vec: DenseVec"""
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x0)
    s = sm.GMRES(tol, iter_max, restart, variant=variant, check_every=check_every)
    s.solve(a, bd, xd)
    assert same(bd.to_numpy(), b)  # (b is read only)
    return results(s, xd.to_numpy())


def run_case(case, dtype, check_every=CHECK_EVERY):
    off, col, val, b, x0 = case.system(dtype)
    tol = case.tol(dtype)
    want = gm.gmres(off, col, val, b, x0, tol, case.iter_max, case.restart)
    a = matrix(off, col, val)
    assert_result(solve_host(a, b, x0, tol, case.iter_max, case.restart), want, (case.name, "host"))
    for ce in check_every:
        assert_result(solve_vec(a, b, x0, tol, case.iter_max, case.restart, ce), want, (case.name, "vec/%d" % ce))
    return want, a, (off, col, val, b, x0)


def ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", gmres_cases.SIZES, ids=ids(gmres_cases.SIZES))
def test_bits_at_every_path_size(gpu, dtype, case):
    """n = 0, 1, 2, 3, 5; 256 .. 259 (every n mod V in one workgroup); 2049 / 2051 (nine workgroups).  GMRES(3), 8 bodies from a
    non-zero x0: three cycles, the last cut short by iter_max (a tiny system exhausts its Krylov space first: breakdown 1 is
    then part of the comparison).  Both entry points, check_every 1, 3 and 8."""
    want, _, _ = run_case(case, dtype)
    assert want.iterations == 8 or case.n <= 5
    if case.n > 5:
        assert want.cycles == 3 and want.breakdown == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_past_the_grid_cap(gpu, dtype):
    """n = 2 * 131 072 * V + 3: the grid is at its cap of 512 workgroups and every thread makes a third trip over the 16-byte
    vectors (the last of them for a few threads only), tails 3 and 1.  GMRES(2), 5 bodies."""
    n = gmres_cases.big_n(dtype)
    off, col, val = bm.tridiag_ns(n, 0.5, dtype, seed=11)
    b, x0 = gmres_cases.rhs(n, dtype, 11)
    want = gm.gmres(off, col, val, b, x0, 0.0, 5, 2)
    assert (want.iterations, want.cycles, want.breakdown) == (5, 3, 0)
    a = matrix(off, col, val)
    assert_result(solve_vec(a, b, x0, 0.0, 5, 2, 3), want, "vec/3")
    assert_result(solve_host(a, b, x0, 0.0, 5, 2), want, "host")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", gmres_cases.RESTARTS, ids=ids(gmres_cases.RESTARTS))
def test_bits_at_restart_lengths_around_the_tile(gpu, dtype, case):
    """restart = 1, 2, tile - 1, tile, tile + 1, 2 tile + 1 and 128 on tridiag(-1, .125, +1) of n = 130, 2 m + 2 bodies: two full cycles
    and a third begun (restart 1: four)."""
    want, _, _ = run_case(case, dtype, check_every=(3, 8))
    assert want.iterations == 2 * case.restart + 2 and want.cycles >= 3 and want.breakdown == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stop_on_tol_inside_a_cycle_on_and_inside_a_batch(gpu, dtype):
    """convdiff2d(5, .5), GMRES(30): the estimate falls under tol in body k < 30 (14 in f32, 23 in f64).  check_every 1, 3 and 8 put
    k inside a replayed batch, check_every = k on a batch boundary.  The stopping body's x update is visible.  Then restart = k:
    the same stop exactly at j = m -- a stop, not a restart: the same bits, one cycle."""
    case = gmres_cases.STOPS[0]
    want, a, (off, col, val, b, x0) = run_case(case, dtype)
    k, tol = want.iterations, case.tol(dtype)
    assert 8 < k < 30 and k % 8 and k % 3 and want.cycles == 1 and want.breakdown == 0 and want.estimates[-1] < tol <= min(want.estimates[:-1])
    before = gm.gmres(off, col, val, b, x0, 0.0, k - 1, 30)
    assert not same(want.x, before.x)
    assert_result(solve_vec(a, b, x0, tol, 200, 30, k), want, "a batch boundary")
    at_m = gm.gmres(off, col, val, b, x0, tol, 200, k)
    assert (at_m.iterations, at_m.cycles) == (k, 1) and same(at_m.x, want.x)
    assert_result(solve_host(a, b, x0, tol, 200, k), at_m, "j = m, host")
    for ce in CHECK_EVERY + (k,):
        assert_result(solve_vec(a, b, x0, tol, 200, k, ce), at_m, ("j = m", ce))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", gmres_cases.STOPS[1:], ids=ids(gmres_cases.STOPS[1:]))
def test_iter_max_ends_the_loop(gpu, dtype, case):
    """tol = 0 on tridiag_ns(259): GMRES(4) with iter_max 11 (inside the third cycle, inside a batch of 3 and of 8) and 8 (at the
    end of the second cycle: a stop, no third cycle begins); GMRES(5) with iter_max 16 (a batch boundary of 8, inside a cycle)."""
    want, _, _ = run_case(case, dtype)
    assert want.iterations == case.iter_max and want.breakdown == 0
    assert want.cycles == {11: 3, 8: 2, 16: 4}[case.iter_max]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_breakdowns_and_iter_max_zero(gpu, dtype):
    """Both codes against the literals of the CPU test and against the model; iter_max = 0 leaves x0 and reports the initial r.r."""
    literal = {"breakdown 1: A = 2 I": ([0.5, 0, 0, 0, 0], 1, 0.0, 1, 1), "breakdown 1: skew 2 x 2": ([0.0, 1.0], 2, 0.0, 1, 1),
               "breakdown 2: b = A x0": ([1.5, 1.0], 0, 0.0, 0, 2), "breakdown 2 with iter_max 0": ([1.5, 1.0], 0, 0.0, 0, 2)}
    for case in gmres_cases.BREAKDOWNS:
        want, a, (off, col, val, b, x0) = run_case(case, dtype, check_every=(0, 2))
        if case.name in literal:
            x, iters, rr, cycles, breakdown = literal[case.name]
            got = solve_host(a, b, x0, case.tol(dtype), case.iter_max, case.restart)
            assert got[0].tolist() == x and got[1:] == (iters, rr, cycles, breakdown), (case.name, got)
        else:
            assert (want.iterations, want.cycles, want.breakdown) == (0, 1, 0) and same(want.x, x0) and want.r_norm_squared > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nan_in_b_runs_to_iter_max(gpu, dtype):
    """NaN compares false everywhere: no stop, no breakdown; GMRES(3) enters all 7 bodies, restarting twice."""
    want, _, _ = run_case(gmres_cases.NONFINITE[0], dtype)
    assert (want.iterations, want.cycles, want.breakdown) == (7, 3, 0) and np.isnan(want.x).all() and math.isnan(want.r_norm_squared)


def test_solves_are_reproducible(gpu):
    for n, dtype, tol in ((257, np.float32, 1e-4), (2049, np.float64, 1e-11)):
        off, col, val, b, x0 = gmres_cases.ns(n, dtype)
        a = matrix(off, col, val)
        first = solve_vec(a, b, x0, tol, 40, 6, 4)
        for other in (solve_vec(a, b, x0, tol, 40, 6, 4), solve_vec(a, b, x0, tol, 40, 6, 5), solve_host(a, b, x0, tol, 40, 6)):
            assert other[1:] == first[1:] and same(other[0], first[0])


# ---- the products ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stream_seq_and_auto_products(gpu, dtype):
    """convdiff2d(12, .5), GMRES(4), 11 bodies from a random x0.  "seq" and "stream" are the oracle's product bit for bit (asserted
    for "stream"), so the model's default product; "auto": the model is fed the device's own checked product."""
    from test_solver_kernels_gpu import device_product
    off, col, val, b, _ = bm.convdiff_system(12, 0.5, dtype)
    x0 = np.random.default_rng(5).uniform(-1, 1, 144).astype(dtype)
    a = matrix(off, col, val)
    want = gm.gmres(off, col, val, b, x0, 0.0, 11, 4)
    assert (want.iterations, want.cycles, want.breakdown) == (11, 3, 0)
    assert same(a.mvp(x0, variant="stream"), oracle.spmv(off, col, val, x0)), "K1s product not bit-exact"
    for variant in ("seq", "stream"):
        assert_result(solve_host(a, b, x0, 0.0, 11, 4, variant), want, (variant, "host"))
        assert_result(solve_vec(a, b, x0, 0.0, 11, 4, 3, variant), want, (variant, "vec/3"))
    auto = gm.gmres(off, col, val, b, x0, 0.0, 11, 4, product=device_product(a, "auto", off, col, val))
    assert_result(solve_host(a, b, x0, 0.0, 11, 4, "auto"), auto, "auto host")
    assert_result(solve_vec(a, b, x0, 0.0, 11, 4, 3, "auto"), auto, "auto vec/3")


FAMILIES = [("k1-lanes8", np.float64), ("k1r-col16", np.float32), ("merge", np.float32), ("colblock", np.float64), ("k1s-xd", np.float32)]


@pytest.mark.parametrize("name,dtype", FAMILIES, ids=["%s-%s" % (n, np.dtype(d).name) for n, d in FAMILIES])
def test_equal_the_model_fed_by_the_checked_device_product(gpu, name, dtype):
    """A few kernel families of tests/kernel_forms.py (the lane-group kernel without and with the ring, merge-path, a column-blocked
    form, K1s), each in the form it is named for: GMRES(4), 11 bodies, the model taking every product -- the initial residual's
    included -- from the device's own eager product of the same variant on the same handle, checked before it is used."""
    from kernel_forms import CONFIGS, env
    from test_solver_kernels_gpu import device_product
    cfg = CONFIGS[name]
    off, col, val = cfg.build(dtype)
    n = len(off) - 1
    rng = np.random.default_rng(1000 + n)
    b, x0 = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
    a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    fused_env = dict(SMH_CG_FUSED_DOT=None, SMH_STREAM_RPT=None) if cfg.fused else {}
    with env(**cfg.env, **fused_env):
        cfg.knobs(a)
        a.prepare(cfg.variant)
        cfg.check(a)
        want = gm.gmres(off, col, val, b, x0, 0.0, 11, 4, product=device_product(a, cfg.variant, off, col, val))
        assert (want.iterations, want.cycles, want.breakdown) == (11, 3, 0) and np.isfinite(want.x).all()
        assert_result(solve_host(a, b, x0, 0.0, 11, 4, cfg.variant), want, (name, "host"))
        assert_result(solve_vec(a, b, x0, 0.0, 11, 4, 4, cfg.variant), want, (name, "vec/4"))
        cfg.check(a)  # (the solves have changed no form)


# ---- where BiCGSTAB gives up ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_skew_dominated_system_where_bicgstab_gives_up(gpu, dtype):
    """tridiag(-1, .125, +1), n = 100, b = A x*: BiCGSTAB on the device does not converge within 400 bodies or breaks down; GMRES(20)
    and GMRES(100) converge -- the model's bits --, and the true residual of their x is below 2 tol."""
    tol = 1e-10 if dtype == np.float64 else 1e-4
    off, col, val, b, _ = gm.skew_system(100, 0.125, dtype)
    x0 = np.zeros(100, dtype)
    a = matrix(off, col, val)
    bi = sm.BiCGStab(tol, 400, variant="seq")
    bi.solve(a, b, x0.copy())
    assert not bi.converged and (bi.breakdown != 0 or bi.iterations == 400), (bi.iterations, bi.breakdown)
    for restart in (20, 100):
        want = gm.gmres(off, col, val, b, x0, tol, 1000, restart)
        assert want.iterations < 1000 and want.estimates[-1] < tol
        got = solve_host(a, b, x0, tol, 1000, restart)
        assert_result(got, want, ("host", restart))
        assert_result(solve_vec(a, b, x0, tol, 1000, restart, 8), want, ("vec/8", restart))
        r = b.astype(np.longdouble) - oracle.spmv(off, col, val.astype(np.float64), got[0].astype(np.float64)).astype(np.longdouble)
        assert float(np.sqrt(np.sum(r * r))) <= 2 * tol


# ---- statuses --------------------------------------------------------------------------------------------------------------------
def status_of(call):
    with pytest.raises(sm.SparseMatPanic) as e:
        call()
    return e.value.status, str(e.value)


def test_statuses_leave_x_untouched(gpu):
    f = np.float64
    off, col, val = bm.tridiag_ns(5, 0.5, f)
    a = matrix(off, col, val)
    wide = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 2], np.ones(2, f))
    s = sm.GMRES(1e-10, 50, variant="seq")
    b5, x5 = np.ones(5, f), np.full(5, 7.0)
    # not square (the family's text), through both entry points
    x2 = np.full(2, 7.0)
    status, text = status_of(lambda: s.solve(wide, np.ones(2, f), x2))
    assert status == _lib.SMH_ERR_NOT_SQUARE and "Matrix is not symmetric" in text and x2.tolist() == [7.0, 7.0]
    xd2 = sm.DenseVec.from_vec(x2)
    assert status_of(lambda: s.solve(wide, sm.DenseVec.from_vec(np.ones(2, f)), xd2))[0] == _lib.SMH_ERR_NOT_SQUARE
    # b_len != n, x_len != n
    status, text = status_of(lambda: s.solve(a, np.ones(4, f), x5))
    assert status == _lib.SMH_ERR_DIM_MISMATCH and "Matrix and vector size mismatch" in text
    x4 = np.full(4, 7.0)
    assert status_of(lambda: s.solve(a, b5, x4))[0] == _lib.SMH_ERR_DIM_MISMATCH
    xd = sm.DenseVec.from_vec(x5)
    assert status_of(lambda: s.solve(a, sm.DenseVec.from_vec(np.ones(6, f)), xd))[0] == _lib.SMH_ERR_DIM_MISMATCH
    # b and x the same storage; a DenseVec of the other dtype
    assert status_of(lambda: s.solve(a, xd, xd))[0] == _lib.SMH_ERR_INVALID
    assert status_of(lambda: s.solve(a, x5, x5))[0] == _lib.SMH_ERR_INVALID
    assert status_of(lambda: s.solve(a, sm.DenseVec.from_vec(np.ones(5, np.float32)), xd))[0] == _lib.SMH_ERR_INVALID
    x32 = sm.DenseVec.from_vec(np.full(5, 7.0, np.float32))
    assert status_of(lambda: s.solve(a, sm.DenseVec.from_vec(b5), x32))[0] == _lib.SMH_ERR_INVALID
    # restart out of range, through both entry points (128 is the last that is taken; 0 stands for 30)
    for form_b, form_x in ((b5, x5), (sm.DenseVec.from_vec(b5), xd)):
        status, text = status_of(lambda: sm.GMRES(1e-10, 50, restart=129, variant="seq").solve(a, form_b, form_x))
        assert status == _lib.SMH_ERR_INVALID and "restart" in text
    # NULL handles and NULL host vectors
    L = sm.lib()
    assert L.smh_gmres_solve_vec(a._h, None, xd._h, 1e-10, 5, 30, 0, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_gmres_solve(None, None, 0, None, 0, 1e-10, 5, 30, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_gmres_solve(a._h, None, 5, x5.ctypes.data, 5, 1e-10, 5, 30, 0, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert x5.tolist() == [7.0] * 5 and x4.tolist() == [7.0] * 4 and x2.tolist() == [7.0] * 2
    assert xd.to_numpy().tolist() == [7.0] * 5 and xd2.to_numpy().tolist() == [7.0] * 2 and x32.to_numpy().tolist() == [7.0] * 5
    assert s.iterations is None and s.cycles is None  # (a refused call reports nothing)
    # ... and the output pointers may be NULL; restart 0 is GMRES(30), 128 is taken
    assert L.smh_gmres_solve_vec(a._h, sm.DenseVec.from_vec(b5)._h, xd._h, 1e-10, 50, 0, _lib.VARIANTS["seq"], 0, None, None, None, None) == 0
    want = gm.gmres(off, col, val, b5, x5, 1e-10, 50, 30)
    assert same(xd.to_numpy(), want.x)
    assert_result(solve_host(a, b5, x5, 1e-10, 50, 128), gm.gmres(off, col, val, b5, x5, 1e-10, 50, 128), "restart 128")
    assert_result(solve_host(a, b5, x5, 1e-10, 50, 0), want, "restart 0")
