"""The device-resident CG (K5: cg.hip with its driver and entry points, blas1.hip's reductions) and the Jacobi-PCG (pcg.hip) pinned
BIT FOR BIT to tests/cg_model.py's restatement of their own summation order: x, r.r (as f64(T)) and the number of entered
bodies -- at the sizes where each code path is first entered (vector tails of every length, fewer elements than lanes, a
second workgroup, a thread's second trip, every grid cap), on unaligned vectors (the VEC=false kernels), from zero and
non-zero x0, stopping on tol in a chosen body and on iter_max inside a replayed batch, and with p.Ap out of the K1s
epilogue on both sides of its first fold.  CG corrects itself, so a tolerance cannot see a stale scalar, a skipped x update
or a lost tail element; equal bits can.

The model (not this file) says what the order is; tests/test_cg_model.py pins the model to the oracle without a GPU."""
import math

import numpy as np
import pytest

import cg_model
import oracle
import sparsemat_amd as sm

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
    """got: (x, iterations, r_norm_squared) of the device; want: a cg_model.Result"""
    x, iters, rr = got
    assert iters == want.iterations, (what, "iterations", iters, want.iterations)
    assert same(np.float64(rr), np.float64(want.r_norm_squared)), (what, "r.r", rr, want.r_norm_squared)
    bad = np.flatnonzero(~((x == want.x) | (np.isnan(x) & np.isnan(want.x))))
    assert same(x, want.x), (what, "x", len(bad), bad[:5], x[bad[:5]], want.x[bad[:5]])


def system(n, dtype, seed=0, spread=0.0, x0_random=False):
    """(off, col, val, b, x0) of the tridiagonal case; b random in [-1, 1], x0 zero or random."""
    off, col, val = cg_model.tridiag(n, dtype, seed=seed, spread=spread)
    return (off, col, val) + rhs(n, dtype, seed, x0_random)


def rhs(n, dtype, seed, x0_random):
    rng = np.random.default_rng(1000 + seed)
    b = rng.uniform(-1, 1, n).astype(dtype)
    x_rand = rng.uniform(-1, 1, n).astype(dtype)
    return b, (x_rand if x0_random else np.zeros(n, dtype))


def matrix(off, col, val):
    n = len(off) - 1
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)


def cg_host(a, b, x0, tol, iter_max, variant="seq"):
    """smh_cg_solve: numpy arrays (check_every is the driver's default, 4)"""
    x = x0.copy()
    s = sm.ConjugateGradient(tol, iter_max, variant=variant)
    s.solve(a, b, x)
    return x, s.iterations, s.r_norm_squared


def cg_vec(a, b, x0, tol, iter_max, check_every, variant="seq"):
    """smh_cg_solve_vec: DenseVec"""
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x0)
    s = sm.ConjugateGradient(tol, iter_max, variant=variant, check_every=check_every)
    s.solve(a, bd, xd)
    return xd.to_numpy(), s.iterations, s.r_norm_squared


def pcg_host(a, b, x0, tol, iter_max, variant="seq"):
    x = x0.copy()
    s = sm.JacobiConjugateGradient(tol, iter_max, variant=variant)
    s.solve(a, b, x)
    return x, s.iterations, s.r_norm_squared


# n: the smallest at which a path is first entered (kBlock = 256 threads, 16-byte vectors of 4 f32 / 2 f64)
#   1, 2, 3, 5, 255, 257     one workgroup; tails of every length (f32: 1, 2, 3, 1, 3, 1; f64: 1, 0, 1, 1, 1, 1), fewer
#                            elements than lanes, lanes without a vector
#   2051 (f32), 2049 (f64)   reduce_blocks = 2: a second workgroup in launch_dot and the CG update sweep; tails 3 and 1
#   131 072 + 259            pcg_grid reaches kPcgBlocks = 512 (514 workgroups asked for); the CG update sweep's 65 workgroups are
#                            on their second (f32) / fourth (f64) trip; tails 3 and 1
#   524 288 + 1027           k_cg_par_p's grid past p_cap (f32: 513 workgroups asked for; f64 since 262 144); PCG's 131 072 threads
#                            stride over 16-byte vectors, so here they make their second trip (f32; third in f64); tails 3 and 1
#   1 048 576 + 2051         the update sweep past its 512-workgroup cap (reduce_blocks = 514); launch_dot still uncapped
SMALL = [1, 2, 3, 5, 255, 257]
LARGE = [131_072 + 259, 524_288 + 1027, 1_048_576 + 2051]


def sizes(dtype):
    return SMALL + [2051 if dtype == np.float32 else 2049] + LARGE


def bodies_for(n):
    return 6 if n < 100_000 else 3


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cg_bits_at_every_path_size(gpu, dtype):
    """Variant "seq", both entry points: numpy arrays (check_every 4: 6 bodies are two replays of the captured batch, the
    second half no-ops) and DenseVec with check_every 7 (plain launches) and 2 (replays)."""
    for k, n in enumerate(sizes(dtype)):
        off, col, val, b, x0 = system(n, dtype, seed=n % 97, x0_random=bool(k % 2))
        a = matrix(off, col, val)
        it = bodies_for(n)
        want = cg_model.cg(off, col, val, b, x0, 0.0, it)
        assert want.iterations == it
        assert_result(cg_host(a, b, x0, 0.0, it), want, ("host", n))
        assert_result(cg_vec(a, b, x0, 0.0, it, 7), want, ("vec/7", n))
        if n < 100_000:
            assert_result(cg_vec(a, b, x0, 0.0, it, 2), want, ("vec/2", n))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pcg_bits_at_every_path_size(gpu, dtype):
    """Variant "seq"; S A S scaling so that d varies (and the plain matrix at the two smallest sizes: d_i = a_ii only)."""
    for k, n in enumerate(sizes(dtype)):
        off, col, val, b, x0 = system(n, dtype, seed=n % 89, spread=0.0 if n < 3 else 2.0, x0_random=not k % 2)
        a = matrix(off, col, val)
        it = 9 if n < 100_000 else 3  # (9: one replayed batch of 8 bodies and one more)
        want = cg_model.pcg(off, col, val, b, x0, 0.0, it)
        assert_result(pcg_host(a, b, x0, 0.0, it), want, ("pcg", n))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_on_a_non_banded_pattern(gpu, dtype):
    """laplace3d(7, 11, 13): n = 1001 (tail 1), seven entries per row, neighbours 1, 7 and 77 rows away."""
    off, col, val = oracle.laplace3d(7, 11, 13, dtype)
    n = 7 * 11 * 13
    a = matrix(off, col, val)
    for x0_random in (False, True):
        b, x0 = rhs(n, dtype, 5, x0_random)
        want = cg_model.cg(off, col, val, b, x0, 0.0, 10)
        assert_result(cg_host(a, b, x0, 0.0, 10), want, ("cg", x0_random))
        assert_result(cg_vec(a, b, x0, 0.0, 10, 3), want, ("cg vec/3", x0_random))
        assert_result(pcg_host(a, b, x0, 0.0, 10), cg_model.pcg(off, col, val, b, x0, 0.0, 10), ("pcg", x0_random))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_past_the_reduction_cap(gpu, dtype):
    """n = 2 097 152 + 2053: reduce_blocks(n) = 1025 -> kReducePartials = 1024 workgroups in launch_dot (threads make a third
    trip in f64), the CG sweeps at their caps, PCG's threads on their 5th (f32) / 9th (f64) trip; tail 1.  Two bodies."""
    n = 2_097_152 + 2053
    assert (n + 2047) // 2048 > cg_model.K_REDUCE_PARTIALS
    x0_random = dtype == np.float32
    off, col, val, b, x0 = system(n, dtype, seed=11, spread=1.0, x0_random=x0_random)
    a = matrix(off, col, val)
    assert_result(cg_host(a, b, x0, 0.0, 2), cg_model.cg(off, col, val, b, x0, 0.0, 2), "cg")
    assert_result(pcg_host(a, b, x0, 0.0, 2), cg_model.pcg(off, col, val, b, x0, 0.0, 2), "pcg")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_system_like_the_oracle(gpu, dtype):
    """n = 0: r.r = 0 < tol after the first body (its alpha is 0 / 0, which nothing reads)."""
    off, col, val = cg_model.tridiag(0, dtype)
    e = np.zeros(0, dtype)
    a = sm.SparseMatCRS.from_raw_parts(0, 0, off, col, val)
    _, o_it, o_rr = oracle.cg(0, 0, off, col, val, e, e, tol=1e-6, iter_max=5)
    _, p_it, p_rr = oracle.pcg_jacobi(0, 0, off, col, val, e, e, tol=1e-6, iter_max=5)
    assert cg_host(a, e, e, 1e-6, 5)[1:] == (o_it, o_rr) == (1, 0.0)
    assert cg_vec(a, e, e, 1e-6, 5, 1)[1:] == (o_it, o_rr)
    assert pcg_host(a, e, e, 1e-6, 5)[1:] == (p_it, p_rr) == (1, 0.0)


def stop_case(solver, dtype):
    """A system, k = 3 and a tol strictly between sqrt(rr_k) and the smallest earlier sqrt(rr): the loop has to leave in body
    k, neither sooner nor later, whatever the batching."""
    n = 2051 if dtype == np.float32 else 2049
    off, col, val, b, x0 = system(n, dtype, seed=21, spread=2.0 if solver == "pcg" else 0.0)
    model = cg_model.cg if solver == "cg" else cg_model.pcg
    full = model(off, col, val, b, x0, 0.0, 8)
    norms = [math.sqrt(float(v)) for v in full.rr_list]
    k = 3
    lo, hi = norms[k - 1], min(norms[:k - 1])
    assert lo < 0.9 * hi, norms  # (the gap the test needs; far wider than any rounding of the square root)
    tol = 0.5 * (lo + hi)
    want = model(off, col, val, b, x0, tol, 50)
    assert want.iterations == k and want.rr == full.rr_list[k - 1]
    assert not same(want.x, model(off, col, val, b, x0, 0.0, k - 1).x)  # (the converging body's x update is visible in x_k)
    return off, col, val, b, x0, tol, k, want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cg_stops_in_exactly_the_converging_body(gpu, dtype):
    """iterations == k, rr == rr_k, x == x_k -- x_k includes the converging body's update -- under graph replay (iter_max >
    check_every) and plain launches, with the stop in the first, a middle and the last body of a batch."""
    off, col, val, b, x0, tol, k, want = stop_case("cg", dtype)
    a = matrix(off, col, val)
    for check_every in (1, 2, 0, 7):
        for iter_max in (k, k + 1, 50):
            assert_result(cg_vec(a, b, x0, tol, iter_max, check_every), want, (check_every, iter_max))
    assert_result(cg_host(a, b, x0, tol, 50), want, "host")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pcg_stops_in_exactly_the_converging_body(gpu, dtype):
    off, col, val, b, x0, tol, k, want = stop_case("pcg", dtype)
    a = matrix(off, col, val)
    for iter_max in (k, 8, 9, 50):
        assert_result(pcg_host(a, b, x0, tol, iter_max), want, iter_max)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_iter_max_ends_the_loop_inside_a_replayed_batch(gpu, dtype):
    """tol = 0: exactly iter_max bodies, also where a replayed batch holds more (the surplus bodies are no-ops on the device);
    iter_max = 0 leaves x untouched and reports the initial r.r."""
    n = 2051 if dtype == np.float32 else 2049
    off, col, val, b, x0 = system(n, dtype, seed=31, spread=1.0, x0_random=True)
    a = matrix(off, col, val)
    for check_every, iter_max in ((4, 5), (4, 8), (7, 9), (1, 3), (4, 0)):
        want = cg_model.cg(off, col, val, b, x0, 0.0, iter_max)
        assert want.iterations == iter_max
        got = cg_vec(a, b, x0, 0.0, iter_max, check_every)
        assert_result(got, want, ("cg", check_every, iter_max))
        if iter_max == 0:
            assert same(got[0], x0) and same(np.float64(got[2]), np.float64(want.rr0))
    for iter_max in (0, 1, 8, 9, 11):
        want = cg_model.pcg(off, col, val, b, x0, 0.0, iter_max)
        got = pcg_host(a, b, x0, 0.0, iter_max)
        assert_result(got, want, ("pcg", iter_max))
        if iter_max == 0:
            assert same(got[0], x0) and same(np.float64(got[2]), np.float64(want.rr0))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [2051, 131_331])
def test_cg_on_unaligned_vectors(gpu, dtype, n):
    """x and / or b one element past a 16-byte boundary (wrapped device pointers): b unaligned sends the RSubInto sweep to
    its VEC=false form (element-wise: no bit can move), x unaligned sends BOTH tail kernels there -- the update sweep's r.r
    then strides over elements, not vectors, which the model restates with aligned=False; launch_dot(r, r) and
    launch_dot(p, Ap) read the solver's own (aligned) buffers and stay vectorised."""
    off, col, val, b, x0 = system(n, dtype, seed=41, x0_random=True)
    a = matrix(off, col, val)
    item = np.dtype(dtype).itemsize
    it = 5
    aligned_model = cg_model.cg(off, col, val, b, x0, 0.0, it)
    unaligned_model = cg_model.cg(off, col, val, b, x0, 0.0, it, aligned=False)
    assert not same(np.array(aligned_model.rr_list), np.array(unaligned_model.rr_list))  # (the two orders do differ here)
    for shift_x, shift_b in ((True, False), (False, True), (True, True)):
        hold_b = sm.DenseVec.from_vec(np.concatenate([np.zeros(1, dtype), b]))
        hold_x = sm.DenseVec.from_vec(np.concatenate([np.zeros(1, dtype), x0]))
        assert hold_b.data_ptr() % 16 == 0 and hold_x.data_ptr() % 16 == 0
        bd = sm.DenseVec.from_device_ptr(hold_b.data_ptr() + item, n, dtype, keep=hold_b) if shift_b else sm.DenseVec.from_vec(b)
        xd = sm.DenseVec.from_device_ptr(hold_x.data_ptr() + item, n, dtype, keep=hold_x) if shift_x else sm.DenseVec.from_vec(x0)
        s = sm.ConjugateGradient(0.0, it, variant="seq", check_every=2)
        s.solve(a, bd, xd)
        got = (xd.to_numpy(), s.iterations, s.r_norm_squared)
        assert_result(got, unaligned_model if shift_x else aligned_model, (shift_x, shift_b))
        if shift_x:
            assert hold_x.to_numpy()[0] == 0  # (the element before x is not the solver's)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_breakdown_of_the_reference(gpu, dtype):
    """b = 0, x0 = 0: alpha = 0 / 0 (no guard, linearsolver.rs:45), x fills with NaN, r.r is NaN, NaN < tol is false:
    iter_max bodies -- as the oracle."""
    n = 257
    off, col, val = cg_model.tridiag(n, dtype, seed=3)
    z = np.zeros(n, dtype)
    a = matrix(off, col, val)
    for got, orc in ((cg_host(a, z, z, 1e-6, 5), oracle.cg), (cg_vec(a, z, z, 1e-6, 5, 2), oracle.cg),
                     (pcg_host(a, z, z, 1e-6, 5), oracle.pcg_jacobi)):
        o_x, o_it, o_rr = orc(n, n, off, col, val, z, z, tol=1e-6, iter_max=5)
        assert got[1] == o_it == 5
        assert np.array_equal(np.isnan(got[0]), np.isnan(o_x)) and np.isnan(o_x).all()
        assert np.isnan(got[2]) and np.isnan(o_rr)


def test_solves_are_reproducible(gpu):
    """Three cases, each solved twice and once more with another check_every: identical bits."""
    for n, dtype, tol in ((257, np.float32, 1e-4), (2049, np.float64, 1e-11), (131_331, np.float32, 0.0)):
        off, col, val, b, x0 = system(n, dtype, seed=51, x0_random=True)
        a = matrix(off, col, val)
        first = cg_vec(a, b, x0, tol, 12, 4)
        for other in (cg_vec(a, b, x0, tol, 12, 4), cg_vec(a, b, x0, tol, 12, 5), cg_host(a, b, x0, tol, 12)):
            assert other[1] == first[1] and same(np.float64(other[2]), np.float64(first[2])) and same(other[0], first[0])
        p1, p2 = pcg_host(a, b, x0, tol, 12), pcg_host(a, b, x0, tol, 12)
        assert p1[1] == p2[1] and same(np.float64(p1[2]), np.float64(p2[2])) and same(p1[0], p2[0])


# The fused p.Ap (variant "stream"): a K1s tile is 256 rows (one row per thread is the default tiling, stream_rpt in crs_forms.hip),
# so spmv_fused_dot_partials returns ceil(n / 256): 9 for n = 2051 / 2049 -- folded by the update's workgroups themselves --
# and 1026 > kReducePartials for n = 262 144 + 259, which enters k_sum_stage1 / k_pcg_sum_stage1.
FUSED_SIZES = [2051, 262_144 + 259]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", FUSED_SIZES)
def test_fused_dot_bits_on_both_sides_of_the_first_fold(gpu, monkeypatch, dtype, n):
    """The K1s epilogue's per-tile order is restated in the model (cg_model.stream_dot_partials: a few lines), so the fused
    path is checked like "seq": bits of x, r.r and the body count, CG through both entry points and PCG.  First the premise:
    K1s's product is the oracle's bit for bit.  Then the same solves with the fused path switched off: the plain model."""
    if dtype == np.float64 and n == 2051:
        n = 2049
    tiles = (n + cg_model.STREAM_TILE_ROWS - 1) // cg_model.STREAM_TILE_ROWS
    assert (tiles > cg_model.K_REDUCE_PARTIALS) == (n > 262_144)
    monkeypatch.delenv("SMH_CG_FUSED_DOT", raising=False)
    monkeypatch.delenv("SMH_STREAM_RPT", raising=False)
    off, col, val, b, x0 = system(n, dtype, seed=61, spread=1.0, x0_random=n > 262_144)
    a = matrix(off, col, val)
    p0 = b - oracle.spmv(off, col, val, x0)
    assert same(a.mvp(p0, variant="stream"), oracle.spmv(off, col, val, p0)), "K1s product not bit-exact"
    it = 5
    fused_cg = cg_model.cg(off, col, val, b, x0, 0.0, it, fused=True)
    fused_pcg = cg_model.pcg(off, col, val, b, x0, 0.0, it, fused=True)
    assert_result(cg_host(a, b, x0, 0.0, it, "stream"), fused_cg, "cg host")
    assert_result(cg_vec(a, b, x0, 0.0, it, 7, "stream"), fused_cg, "cg vec/7")
    assert_result(pcg_host(a, b, x0, 0.0, it, "stream"), fused_pcg, "pcg")
    monkeypatch.setenv("SMH_CG_FUSED_DOT", "0")  # (read per call)
    assert_result(cg_host(a, b, x0, 0.0, it, "stream"), cg_model.cg(off, col, val, b, x0, 0.0, it), "cg, separate dot")
    assert_result(pcg_host(a, b, x0, 0.0, it, "stream"), cg_model.pcg(off, col, val, b, x0, 0.0, it), "pcg, separate dot")
