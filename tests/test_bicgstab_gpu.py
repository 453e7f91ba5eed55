"""The device-resident BiCGSTAB (bicgstab.hip) pinned BIT FOR BIT to tests/bicgstab_model.py's "device" mode: x, the number of
entered bodies, f64(rr) and the breakdown code -- at the sizes where each path of the sweeps is first entered, through both
entry points, under plain launches and graph replay, stopping at the half step and at the full step in the middle of a batch,
on iter_max inside a batch, on every breakdown, on the empty system.  Variant "seq" (and "stream", whose product is the
oracle's bit for bit too); "auto" is held to the accuracy the model reaches.

The model (not this file) says what the arithmetic is; tests/test_bicgstab_model.py pins the model without a GPU."""
import numpy as np
import pytest

import bicgstab_model as bm
import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]


def same(a, b):
    """bit equality (any NaN equals any NaN: its sign and payload are not arithmetic)"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def assert_result(got, want, what):
    """got: (x, iterations, r_norm_squared, breakdown, converged) of the device; want: a bicgstab_model.Result"""
    x, iters, rr, breakdown, converged = got
    assert iters == want.iterations, (what, "iterations", iters, want.iterations)
    assert breakdown == want.breakdown, (what, "breakdown", breakdown, want.breakdown)
    assert same(np.float64(rr), np.float64(want.r_norm_squared)), (what, "r.r", rr, want.r_norm_squared)
    bad = np.flatnonzero(~((x == want.x) | (np.isnan(x) & np.isnan(want.x))))
    assert same(x, want.x), (what, "x", len(bad), bad[:5], x[bad[:5]], want.x[bad[:5]])
    assert converged is want.converged, (what, "converged", converged, want.converged)


def rhs(n, dtype, seed, x0_random):
    rng = np.random.default_rng(1000 + seed)
    b = rng.uniform(-1, 1, n).astype(dtype)
    x_rand = rng.uniform(-1, 1, n).astype(dtype)
    return b, (x_rand if x0_random else np.zeros(n, dtype))


def matrix(off, col, val):
    n = len(off) - 1
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)


def results(s, x):
    return x, s.iterations, s.r_norm_squared, s.breakdown, s.converged


def solve_host(a, b, x0, tol, iter_max, variant="seq"):
    """smh_bicgstab_solve: numpy arrays (check_every is the driver's default, 8)"""
    x = x0.copy()
    s = sm.BiCGStab(tol, iter_max, variant=variant)
    s.solve(a, b, x)
    return results(s, x)


def solve_vec(a, b, x0, tol, iter_max, check_every, variant="seq"):
    """smh_bicgstab_solve_vec: DenseVec"""
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x0)
    s = sm.BiCGStab(tol, iter_max, variant=variant, check_every=check_every)
    s.solve(a, bd, xd)
    assert same(bd.to_numpy(), b)  # (b is read only)
    return results(s, xd.to_numpy())


# n: the smallest at which a path of the sweeps is first entered (kBlock = 256 threads, 16-byte vectors of 4 f32 / 2 f64)
#   1, 2, 3, 5, 255, 257     one workgroup; tails of every length (f32: 1, 2, 3, 1, 3, 1; f64: 1, 0, 1, 1, 1, 1), fewer elements
#                            than lanes, lanes without a vector
#   2051 (f32), 2049 (f64)   several workgroups (9); tails 3 and 1
#   131 072 + 259            the grid reaches its cap of 512 workgroups (514 asked for); tails 3 and 1
#   524 288 + 1027           131 072 threads stride over 16-byte vectors: their second trip (f32; third in f64); tails 3 and 1
def sizes(dtype):
    return [1, 2, 3, 5, 255, 257, 2051 if dtype == np.float32 else 2049, 131_072 + 259, 524_288 + 1027]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_at_every_path_size(gpu, dtype):
    """tol 0: 9 bodies below 100 000 rows (the host entry: one replayed batch of 8 and one more), 3 above (plain launches).
    Both entry points; DenseVec with check_every 7 (plain launches) and 2 (replays; 3 bodies replay 4, the last a no-op).  A breakdown that the model meets at a
    tiny size (n = 1: the first body solves the system) is part of the comparison."""
    for k, n in enumerate(sizes(dtype)):
        off, col, val = bm.tridiag_ns(n, 0.5, dtype, seed=n % 97)
        b, x0 = rhs(n, dtype, n % 97, bool(k % 2))
        a = matrix(off, col, val)
        it = 9 if n < 100_000 else 3
        want = bm.bicgstab(off, col, val, b, x0, 0.0, it)
        assert want.iterations == it or n < 10
        assert_result(solve_host(a, b, x0, 0.0, it), want, ("host", n))
        assert_result(solve_vec(a, b, x0, 0.0, it, 7), want, ("vec/7", n))
        assert_result(solve_vec(a, b, x0, 0.0, it, 2), want, ("vec/2", n))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_on_a_non_banded_pattern(gpu, dtype):
    """convdiff2d(23, .25): n = 529 (tail 1), five entries per row, neighbours 1 and 23 rows away, the diagonal stored first."""
    off, col, val = bm.convdiff2d(23, 0.25, dtype)
    a = matrix(off, col, val)
    for x0_random in (False, True):
        b, x0 = rhs(23 * 23, dtype, 5, x0_random)
        want = bm.bicgstab(off, col, val, b, x0, 0.0, 10)
        assert want.iterations == 10 and want.breakdown == 0
        assert_result(solve_host(a, b, x0, 0.0, 10), want, ("host", x0_random))
        assert_result(solve_vec(a, b, x0, 0.0, 10, 3), want, ("vec/3", x0_random))


# convdiff2d(8, c), b = A x*, x0 = 0, tol 1e-10 (f64) / 1e-4 (f32): chosen from the model -- c = 1 stops at the half step
# (body 23 in f64, 13 in f32), c = .5 at the full step (body 25 / 13): odd bodies, so never the last of a batch of 2 or 8
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c,half", [(1.0, True), (0.5, False)], ids=["half-step", "full-step"])
def test_stops_in_exactly_the_stopping_body(gpu, dtype, c, half):
    tol = 1e-10 if dtype == np.float64 else 1e-4
    off, col, val, b, _ = bm.convdiff_system(8, c, dtype)
    x0 = np.zeros(64, dtype)
    want = bm.bicgstab(off, col, val, b, x0, tol, 200)
    k = want.iterations
    assert want.converged and want.half_step is half and k % 2 == 1 and 8 < k < 100, (k, want.half_step)
    before = bm.bicgstab(off, col, val, b, x0, 0.0, k - 1)
    assert not same(want.x, before.x)  # (the stopping body's x update is visible in x_k)
    a = matrix(off, col, val)
    for check_every in (2, 8):
        assert_result(solve_vec(a, b, x0, tol, 200, check_every), want, check_every)
    assert_result(solve_host(a, b, x0, tol, 200), want, "host")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_iter_max_ends_the_loop_inside_a_replayed_batch(gpu, dtype):
    """tol = 0: exactly iter_max bodies where the replayed batch holds 8 (the surplus bodies are no-ops on the device)."""
    n = 2051 if dtype == np.float32 else 2049
    off, col, val = bm.tridiag_ns(n, 0.5, dtype, seed=31)
    b, x0 = rhs(n, dtype, 31, True)
    a = matrix(off, col, val)
    want = bm.bicgstab(off, col, val, b, x0, 0.0, 5)
    assert want.iterations == 5 and want.breakdown == 0 and not want.converged
    assert_result(solve_vec(a, b, x0, 0.0, 5, 8), want, "vec/8")
    # (9 bodies, batches of 4: the third replay runs one body and three no-ops)
    assert_result(solve_vec(a, b, x0, 0.0, 9, 4), bm.bicgstab(off, col, val, b, x0, 0.0, 9), "vec/4")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cases_on_the_device(gpu, dtype):
    """Every breakdown code, the half-step stop and iter_max = 0, against the literals of the CPU test and against the model."""
    for name, a_dense, b, iters, x, rr, breakdown, converged in bm.EXACT:
        off, col, val = bm.dense_to_crs(a_dense, dtype)
        b, x0 = np.array(b, dtype), np.zeros(len(b), dtype)
        a = matrix(off, col, val)
        want = bm.bicgstab(off, col, val, b, x0, 1e-6, 10)
        for got in (solve_host(a, b, x0, 1e-6, 10), solve_vec(a, b, x0, 1e-6, 10, 2), solve_vec(a, b, x0, 1e-6, 10, 0)):
            assert_result(got, want, name)
            assert got[0].tolist() == x and got[1:] == (iters, rr, breakdown, converged), (name, got)
    off, col, val = bm.dense_to_crs([[2, 1], [0, 3]], dtype)
    a = matrix(off, col, val)
    b, x0 = np.array([5, 4], dtype), np.array([1.5, 1.0], dtype)
    for got in (solve_host(a, b, x0, 1e-6, 0), solve_vec(a, b, x0, 1e-6, 0, 3)):
        assert got[0].tolist() == [1.5, 1.0] and got[1:] == (0, 2.0, 0, False), got


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_system(gpu, dtype):
    """n = 0: rho = 0, so the first body breaks down with code 2; iter_max = 0 enters none."""
    off, col, val = bm.tridiag_ns(0, 0.5, dtype)
    e = np.zeros(0, dtype)
    a = sm.SparseMatCRS.from_raw_parts(0, 0, off, col, val)
    for iter_max, iters, breakdown in ((3, 1, 2), (0, 0, 0)):
        want = bm.bicgstab(off, col, val, e, e, 1e-6, iter_max)
        assert (want.iterations, want.r_norm_squared, want.breakdown, want.converged) == (iters, 0.0, breakdown, False)
        assert_result(solve_host(a, e, e, 1e-6, iter_max), want, ("host", iter_max))
        assert_result(solve_vec(a, e, e, 1e-6, iter_max, 2), want, ("vec", iter_max))


def test_solves_are_reproducible(gpu):
    for n, dtype, tol in ((257, np.float32, 1e-4), (2049, np.float64, 1e-11), (131_331, np.float32, 0.0)):
        off, col, val = bm.tridiag_ns(n, 0.5, dtype, seed=51)
        b, x0 = rhs(n, dtype, 51, True)
        a = matrix(off, col, val)
        first = solve_vec(a, b, x0, tol, 12, 4)
        for other in (solve_vec(a, b, x0, tol, 12, 4), solve_vec(a, b, x0, tol, 12, 5), solve_host(a, b, x0, tol, 12)):
            assert other[1:] == first[1:] and same(other[0], first[0])


def status_of(call):
    with pytest.raises(sm.SparseMatPanic) as e:
        call()
    return e.value.status, str(e.value)


def test_statuses_leave_x_untouched(gpu):
    f = np.float64
    off, col, val = bm.tridiag_ns(5, 0.5, f)
    a = matrix(off, col, val)
    wide = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 2], np.ones(2, f))
    s = sm.BiCGStab(1e-10, 50, variant="seq")
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
    # b and x the same DenseVec; a DenseVec of the other dtype
    assert status_of(lambda: s.solve(a, xd, xd))[0] == _lib.SMH_ERR_INVALID
    assert status_of(lambda: s.solve(a, sm.DenseVec.from_vec(np.ones(5, np.float32)), xd))[0] == _lib.SMH_ERR_INVALID
    x32 = sm.DenseVec.from_vec(np.full(5, 7.0, np.float32))
    assert status_of(lambda: s.solve(a, sm.DenseVec.from_vec(b5), x32))[0] == _lib.SMH_ERR_INVALID
    # NULL handles
    L = sm.lib()
    assert L.smh_bicgstab_solve_vec(a._h, None, xd._h, 1e-10, 5, 0, 0, None, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_bicgstab_solve(None, None, 0, None, 0, 1e-10, 5, 0, None, None, None) == _lib.SMH_ERR_INVALID
    assert x5.tolist() == [7.0] * 5 and x4.tolist() == [7.0] * 4 and x2.tolist() == [7.0] * 2
    assert xd.to_numpy().tolist() == [7.0] * 5 and xd2.to_numpy().tolist() == [7.0] * 2 and x32.to_numpy().tolist() == [7.0] * 5
    assert s.iterations is None  # (a refused call reports nothing)
    # ... and the output pointers may be NULL
    assert L.smh_bicgstab_solve_vec(a._h, sm.DenseVec.from_vec(b5)._h, xd._h, 1e-10, 50, _lib.VARIANTS["seq"], 0, None, None, None) == 0
    want = bm.bicgstab(off, col, val, b5, x5, 1e-10, 50)
    assert same(xd.to_numpy(), want.x)


def test_auto_and_stream_variants(gpu):
    """convdiff2d(12, .5) in f64, tol 1e-10.  "auto": converged without a breakdown, max|x - x*| <= 1e-8 (the model's own
    bound, test_bicgstab_model.py).  "stream": K1s's product is the oracle's bit for bit and this solver takes nothing from
    its epilogue, so the model's bits."""
    off, col, val, b, x_star = bm.convdiff_system(12, 0.5, np.float64)
    x0 = np.zeros(144)
    a = matrix(off, col, val)
    x, iters, rr, breakdown, converged = solve_host(a, b, x0, 1e-10, 200, "auto")
    err = float(np.abs(x - x_star).max())
    print("auto:", iters, rr, breakdown, err)
    assert converged and breakdown == 0 and iters < 200 and np.sqrt(rr) < 1e-10
    assert err <= 1e-8
    p0 = b - oracle.spmv(off, col, val, x_star * 0.5)
    assert same(a.mvp(p0, variant="stream"), oracle.spmv(off, col, val, p0)), "K1s product not bit-exact"
    want = bm.bicgstab(off, col, val, b, x0, 1e-10, 200)
    assert_result(solve_host(a, b, x0, 1e-10, 200, "stream"), want, "stream host")
    assert_result(solve_vec(a, b, x0, 1e-10, 200, 3, "stream"), want, "stream vec/3")
