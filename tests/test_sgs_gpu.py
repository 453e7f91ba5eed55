"""GPU: the symmetric Gauss-Seidel preconditioner (smh_crs_sgs_apply_vec) and its CG (smh_pcg_sgs_solve*, csrc/pcg.hip over
csrc/trisolve.hip) pinned BIT FOR BIT to tests/sgs_model.py in "device" mode: x, the number of entered bodies and f64(r.r), on
the four grid cases of the model's table in the natural and the red-black ordering, through the STREAM product (p.Ap out of
its epilogue), SEQ and AUTO.  The model takes every product from the device's own product of the same variant on the same
handle, held to the suite's parity bound against the oracle first (as tests/test_solver_kernels_gpu.py does), so no tolerance
appears in the solver cases.  The table's grids are multiples of 4 inside one trip of the sweeps' grid: the path sizes further down
(n = 3, 391 and 262 447) run the tails, a second workgroup and a thread's second trip, for tests/test_ilu_gpu.py too."""
import math
import os

import numpy as np
import pytest

import cg_model
import sgs_model as sg
import sparsemat_amd as sm
import trisolve_model as tm
from kernel_forms import env, same
from sparsemat_amd import _lib
from util import assert_spmv_close

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ORDERINGS = ["natural", "red_black"]


def handle(off, col, val):
    n = len(off) - 1
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)


def device_product(m, variant, off, col, val):
    seen = {}

    def product(v):
        v = np.ascontiguousarray(v, val.dtype)
        key = v.tobytes()
        if key not in seen:
            y = m.mvp(v, variant=variant)
            assert_spmv_close(y, off, col, val, v, "solver product, variant %s" % variant)
            seen[key] = y
        return seen[key].copy()
    return product


def is_fused(m, variant):
    return variant == "stream" or (variant == "auto" and m.resolved_variant()[0] == "stream")


def run_host(m, b, x0, tol, iter_max, variant):
    s = sm.SGSConjugateGradient(tol, iter_max, variant=variant)
    x = x0.copy()
    s.solve(m, b, x)
    return x, s.iterations, np.float64(s.r_norm_squared)


def run_vec(m, b, x0, tol, iter_max, variant, check_every):
    s = sm.SGSConjugateGradient(tol, iter_max, variant=variant, check_every=check_every)
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x0)
    s.solve(m, bd, xd)
    assert same(bd.to_numpy(), b)
    return xd.to_numpy(), s.iterations, np.float64(s.r_norm_squared)


def assert_result(got, want, what):
    x, iters, rr = got
    assert iters == want.iterations, (what, "bodies", iters, want.iterations)
    assert same(rr, np.float64(want.r_norm_squared)), (what, "r.r", rr, want.r_norm_squared)
    bad = np.flatnonzero(x != want.x)
    assert same(x, want.x), (what, "x", len(bad), bad[:5], x[bad[:5]], want.x[bad[:5]])


_SYSTEMS = {}


def system(k, ordering):
    """table case k with its handle-independent data, computed once"""
    if (k, ordering) not in _SYSTEMS:
        _SYSTEMS[k, ordering] = sg.table_case(k, ordering)
    return _SYSTEMS[k, ordering]


@pytest.mark.parametrize("ordering", ORDERINGS)
@pytest.mark.parametrize("k", range(len(sg.TABLE)))
def test_apply_equals_the_model(gpu, k, ordering):
    off, col, val, r, _ = system(k, ordering)
    a = handle(off, col, val)
    want = sg.sgs_apply(off, col, val, r, (tm.Plan(off, col, tm.LOWER), tm.Plan(off, col, tm.UPPER)))
    got = a.sgs_apply(r)
    assert same(got, want), np.flatnonzero(got != want)[:5]
    rd = sm.DenseVec.from_vec(r)
    assert same(a.sgs_apply(rd).to_numpy(), want) and same(rd.to_numpy(), r)
    _lib.check(sm.lib().smh_crs_sgs_apply_vec(a._h, rd._h, rd._h))  # z may be r
    assert same(rd.to_numpy(), want)
    assert a.trisolve_levels("lower")["n_levels"] == a.trisolve_levels("upper")["n_levels"] == (2 if ordering == "red_black" else sum(sg.TABLE[k][:2]) - 1)
    # M z = r, recomputed in f64: the bound of tests/test_sgs_model.py::test_apply_inverts_m (3 gamma_6 |D + L| |D^-1| |D + U| |z|)
    n = len(r)
    A = np.zeros((n, n))
    np.add.at(A, (np.repeat(np.arange(n), np.diff(off.astype(np.int64))), col.astype(np.int64)), val.astype(np.float64))
    D, L, U, Dinv = np.diag(np.diag(A)), np.tril(A, -1), np.triu(A, 1), np.diag(1.0 / np.diag(A))
    u = 2.0 ** (-24 if val.dtype == F32 else -53)
    z = got.astype(np.float64)
    bound = 1.1 * 3 * 6 * u * (np.abs(D + L) @ Dinv @ np.abs(D + U)) @ np.abs(z)
    assert (np.abs((D + L) @ Dinv @ (D + U) @ z - r.astype(np.float64)) <= bound).all()


@pytest.mark.parametrize("variant", ["stream", "seq", "auto"])
@pytest.mark.parametrize("ordering", ORDERINGS)
@pytest.mark.parametrize("k", range(len(sg.TABLE)))
def test_solve_equals_the_model_fed_by_the_device_product(gpu, k, ordering, variant):
    """To the table's tolerance from x0 = 0: the body count, x and r.r of the model -- and the count under 0.6 of Jacobi's on the
    device too.  Host vectors (check_every: the default, 8) and device vectors with check_every 3."""
    off, col, val, b, tol = system(k, ordering)
    n = len(b)
    a = handle(off, col, val)
    a.prepare(variant)
    x0 = np.zeros(n, val.dtype)
    product = device_product(a, variant, off, col, val)
    want = sg.sgs_pcg(off, col, val, b, x0, tol, 500, fused=is_fused(a, variant), product=product)
    assert 10 < want.iterations < 120 and math.sqrt(want.r_norm_squared) < tol
    assert_result(run_host(a, b, x0, tol, 500, variant), want, (k, ordering, variant, "host"))
    assert_result(run_vec(a, b, x0, tol, 500, variant, 3), want, (k, ordering, variant, "vec/3"))
    if variant == "auto":
        jac = sm.JacobiConjugateGradient(tol, 2000)
        jac.solve(a, b, x0.copy())
        assert want.iterations < 0.6 * jac.iterations, (want.iterations, jac.iterations)


@pytest.mark.parametrize("dtype", [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")])
def test_stops_batches_and_iter_max(gpu, dtype):
    """From a random x0 with tol = 0 and iter_max = 11 (an iter_max inside a batch of 3, of 8 and of the host default; check_every
    1, 3 and 8), then stops on tol inside a replayed batch and on a batch boundary, each twice on the same handle; iter_max =
    0; b = 0."""
    k = 3 if dtype == F32 else 1
    off, col, val, b, _ = system(k, "red_black")
    n = len(b)
    a = handle(off, col, val)
    x0 = np.random.default_rng(7).uniform(-1, 1, n).astype(dtype)
    product = device_product(a, "stream", off, col, val)
    model = lambda tol, iter_max, bb=b, xx=x0: sg.sgs_pcg(off, col, val, bb, xx, tol, iter_max, fused=True, product=product)
    want = model(0.0, 11)
    assert want.iterations == 11 and np.isfinite(want.x).all()
    for attempt in range(2):
        assert_result(run_host(a, b, x0, 0.0, 11, "stream"), want, ("iter_max", "host", attempt))
        for ce in (1, 3, 8):
            assert_result(run_vec(a, b, x0, 0.0, 11, "stream", ce), want, ("iter_max", ce, attempt))
    # a tolerance that body j is the first to undercut: between its norm and the smallest before it.  Every such body from the
    # fourth on is stopped at with batches of 1, 3 and 8 bodies; among them a stop inside a replayed batch and one on its boundary
    norms = [math.sqrt(float(v)) for v in want.rr_list]
    kinds = set()
    for body in range(4, 11):
        before = min(norms[:body - 1])
        if not norms[body - 1] < 0.95 * before:
            continue
        tol = 0.5 * (norms[body - 1] + before)
        stopped = model(tol, 50)
        assert stopped.iterations == body and not same(stopped.x, model(0.0, body - 1).x)
        for ce in (1, 3, 8):
            for attempt in range(2):
                assert_result(run_vec(a, b, x0, tol, 50, "stream", ce), stopped, ("stop", body, ce, attempt))
            if ce > 1:
                kinds.add("boundary" if body % ce == 0 else "inside")
        assert_result(run_host(a, b, x0, tol, 50, "stream"), stopped, ("stop", body, "host"))
    assert kinds == {"boundary", "inside"}, (kinds, norms)
    none = model(0.0, 0)
    assert_result(run_host(a, b, x0, 0.0, 0, "stream"), none, "iter_max 0")
    assert_result(run_vec(a, b, x0, 0.0, 0, "stream", 3), none, "iter_max 0, vec")
    zero = np.zeros(n, dtype)
    nan = model(1e-10, 9, zero, zero)
    assert nan.iterations == 9 and np.isnan(nan.x).all()
    assert_result(run_vec(a, zero, zero, 1e-10, 9, "stream", 4), nan, "b = 0")


@pytest.mark.parametrize("dtype", [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")])
def test_node_budget_changes_no_bit(gpu, dtype):
    """The red-black 64 x 65 grid: two levels of 2080 rows, so 2 launches per solve, 4 per application and some 16 nodes per
    body.  With the budget of a captured batch lowered to 40 nodes (SMH_SGS_GRAPH_NODES) batches of 8 bodies become batches of 2;
    lowered to 8 nodes a single body is beyond it and the loop runs uncaptured.  Both give the bits of the replayed route."""
    off, col, val = sg.lap2d(64, 65, dtype, seed=2, spread=1.0)
    off, col, val = sg.permute_symmetric(off, col, val, sg.red_black(64, 65))
    n = len(off) - 1
    a = handle(off, col, val)
    assert a.trisolve_levels("lower")["n_launches"] == 2 and a.trisolve_levels("upper")["n_launches"] == 2
    rng = np.random.default_rng(3)
    b, x0 = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
    product = device_product(a, "stream", off, col, val)
    want = sg.sgs_pcg(off, col, val, b, x0, 0.0, 13, fused=True, product=product)
    norms = [math.sqrt(float(v)) for v in want.rr_list]
    body = next(j for j in range(5, 13) if norms[j - 1] < 0.95 * min(norms[:j - 1]))
    tol = 0.5 * (norms[body - 1] + min(norms[:body - 1]))
    stopped = sg.sgs_pcg(off, col, val, b, x0, tol, 50, fused=True, product=product)
    assert stopped.iterations == body
    for nodes in (None, "40", "8"):
        with env(SMH_SGS_GRAPH_NODES=nodes):
            assert_result(run_vec(a, b, x0, 0.0, 13, "stream", 8), want, ("budget", nodes))
            assert_result(run_vec(a, b, x0, tol, 50, "stream", 8), stopped, ("budget, stop", nodes))
            assert_result(run_host(a, b, x0, tol, 50, "stream"), stopped, ("budget, host", nodes))


# ---- every path of the sweeps (k_sgs_dot, k_sgs_update, k_sgs_p and the fold) -------------------------------------------------
# (nx, ny, spread, ordering, bodies).  The sweeps take 16 bytes per lane and then the last n % V rows one by one (V = 4 in f32, 2 in
# f64), on min(ceil(n / 256), 512) workgroups.  n = 3: no whole vector in f32, one vector and one tail row in f64.  n = 391: two
# workgroups, a tail of 3 (f32) and of 1 (f64); nine bodies are a replayed batch of 8 and one more.
SMALL_PATHS = [(1, 3, 0.0, "natural", 2), (23, 17, 1.0, "natural", 9), (23, 17, 1.0, "red_black", 9)]
# n = 262 447: the grid is at its cap, 131 072 threads over 131 223 f64 vectors, so threads make a second trip; the tail is 1.
# Red-black keeps the schedules at two levels (the model solves level by level).  f32 makes a second trip only past 524 288 rows.
BIG_PATH = (361, 727, 1.0, "red_black", 3)
_PATHS = {}


def path_system(nx, ny, spread, ordering, dtype):
    """(off, col, val, b, x0) of lap2d(nx, ny) in the ordering, b and x0 random, computed once"""
    key = nx, ny, spread, ordering, np.dtype(dtype).name
    if key not in _PATHS:
        off, col, val = sg.lap2d(nx, ny, dtype, seed=2, spread=spread)
        if ordering == "red_black":
            off, col, val = sg.permute_symmetric(off, col, val, sg.red_black(nx, ny))
        rng = np.random.default_rng(11)
        n = nx * ny
        _PATHS[key] = off, col, val, rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
    return _PATHS[key]


def path_ids(cases):
    return ["%dx%d-%s" % (c[0], c[1], c[3]) for c in cases]


def check_path(case, dtype, precond=None, run_host=None, run_vec=None):
    """tol = 0 from a random x0 through the STREAM product: the model's bits from the host entry and from the _vec entry with
    check_every 3.  run_host / run_vec: (handle, b, x0, tol, iter_max, variant[, check_every]) -> (x, bodies, r.r)"""
    nx, ny, spread, ordering, bodies = case
    off, col, val, b, x0 = path_system(nx, ny, spread, ordering, dtype)
    a = handle(off, col, val)
    want = sg.sgs_pcg(off, col, val, b, x0, 0.0, bodies, fused=True, product=device_product(a, "stream", off, col, val), precond=precond)
    assert want.iterations == bodies and np.isfinite(want.x).all() and np.isfinite(want.r_norm_squared)
    assert_result(run_host(a, b, x0, 0.0, bodies, "stream"), want, (case, "host"))
    assert_result(run_vec(a, b, x0, 0.0, bodies, "stream", 3), want, (case, "vec/3"))


@pytest.mark.parametrize("dtype", [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")])
@pytest.mark.parametrize("case", SMALL_PATHS, ids=path_ids(SMALL_PATHS))
def test_bits_at_every_path_size(gpu, case, dtype):
    n, V = case[0] * case[1], 16 // np.dtype(dtype).itemsize
    assert (n, n % V) in ((3, 3), (3, 1), (391, 3), (391, 1))
    check_path(case, dtype, None, run_host, run_vec)


def test_bits_on_a_second_trip_of_the_grid(gpu):
    nx, ny = BIG_PATH[:2]
    assert nx * ny // 2 > 512 * 256 and (nx * ny) % 2 == 1
    check_path(BIG_PATH, F64, None, run_host, run_vec)


def test_statuses(gpu):
    L = sm.lib()
    off, col, val, b, tol = system(3, "natural")
    n = len(b)
    a = handle(off, col, val)
    x = np.zeros(n, F32)
    solver = sm.SGSConjugateGradient(tol, 50)

    def status_of(call):
        with pytest.raises(_lib.SparseMatPanic) as e:
            call()
        return e.value.status, str(e.value)

    # a zero diagonal value and an absent diagonal entry: refused, the row named (as Jacobi's)
    pos = tm.diag_positions(off, col)
    v0 = val.copy()
    v0[pos[37]] = 0.0
    st, msg = status_of(lambda: solver.solve(handle(off, col, v0), b, x))
    assert st == _lib.SMH_ERR_INVALID and "row 37" in msg
    keep = np.ones(len(col), bool)
    keep[pos[[41, 99]]] = False
    o2 = np.zeros(n + 1, np.uint32)
    o2[1:] = np.cumsum(np.add.reduceat(keep.astype(np.int64), off[:-1].astype(np.int64)))
    nodiag = handle(o2, col[keep], val[keep])
    st, msg = status_of(lambda: solver.solve(nodiag, b, x))
    assert st == _lib.SMH_ERR_INVALID and "row 41" in msg
    st, msg = status_of(lambda: solver.solve(nodiag, sm.DenseVec.from_vec(b), sm.DenseVec.zeros(n, F32)))
    assert st == _lib.SMH_ERR_INVALID and "row 41" in msg
    st, msg = status_of(lambda: nodiag.sgs_apply(b))
    assert st == _lib.SMH_ERR_INVALID and "row 41" in msg
    assert not x.any()
    # not square, dimension mismatch
    rect = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 1], np.ones(2, F32))
    assert status_of(lambda: solver.solve(rect, np.ones(2, F32), np.zeros(2, F32)))[0] == _lib.SMH_ERR_NOT_SQUARE
    assert status_of(lambda: solver.solve(rect, sm.DenseVec.zeros(2, F32), sm.DenseVec.zeros(2, F32)))[0] == _lib.SMH_ERR_NOT_SQUARE
    assert status_of(lambda: rect.sgs_apply(np.ones(2, F32)))[0] == _lib.SMH_ERR_NOT_SQUARE
    assert status_of(lambda: solver.solve(a, b[:-1], x))[0] == _lib.SMH_ERR_DIM_MISMATCH
    assert status_of(lambda: solver.solve(a, b, np.zeros(n + 1, F32)))[0] == _lib.SMH_ERR_DIM_MISMATCH
    assert status_of(lambda: solver.solve(a, sm.DenseVec.from_vec(b), sm.DenseVec.zeros(n - 1, F32)))[0] == _lib.SMH_ERR_DIM_MISMATCH
    assert status_of(lambda: a.sgs_apply(b[:-1]))[0] == _lib.SMH_ERR_DIM_MISMATCH
    # invalid arguments of the raw entry points
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.zeros(n, F32)
    assert L.smh_pcg_sgs_solve(None, None, 0, None, 0, 1e-6, 10, 0, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_sgs_solve(a._h, None, n, x.ctypes.data, n, 1e-6, 10, 0, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_sgs_solve_vec(a._h, None, xd._h, 1e-6, 10, 0, 0, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_sgs_solve_vec(a._h, bd._h, bd._h, 1e-6, 10, 0, 0, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_pcg_sgs_solve_vec(a._h, bd._h, sm.DenseVec.zeros(n, F64)._h, 1e-6, 10, 0, 0, None, None) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_sgs_apply_vec(a._h, None, xd._h) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_sgs_apply_vec(a._h, bd._h, sm.DenseVec.zeros(n, F64)._h) == _lib.SMH_ERR_INVALID
    # the output pointers may be NULL, and the good handle still solves
    assert L.smh_pcg_sgs_solve_vec(a._h, bd._h, xd._h, tol, 50, 0, 0, None, None) == _lib.SMH_OK
    want = sg.sgs_pcg(off, col, val, b, x, tol, 50, fused=is_fused(a, "auto"), product=device_product(a, "auto", off, col, val))
    assert same(xd.to_numpy(), want.x)
    # no rows: nothing to do
    z = sm.SparseMatCRS.from_raw_parts(0, 0, [0], [], np.zeros(0, F32))
    e = np.zeros(0, F32)
    solver.solve(z, e, e.copy())
    assert solver.iterations == 1  # (the empty r.r is 0: the first body's stop test passes)
    assert len(z.sgs_apply(e)) == 0
