"""The k-column conjugate gradient (K5m: cg_many.hip behind smh_cg_solve_many) pinned BIT FOR BIT to tests/cg_many_model.py:
x, the number of entered bodies and r.r (as f64(T)) of every column -- at the sizes where each path is first entered, for k
with and without padding and on both sides of a row group, from zero and non-zero x0, with columns that stop in different
bodies, a NaN recurrence beside finite ones, iter_max inside a replayed batch, and every status.

The model runs the columns one after the other, so it cannot let one column reach another; equal bits on the device say that
it does not either.  tests/test_cg_many_model.py pins the model to the oracle without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import cg_many_model
import cg_model
import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
# n: 1, 2, 3, 5 fewer rows than lanes; 255, 257 one workgroup, a ragged last wave / a second trip of thread 0; 2051: a second
# workgroup (reduce_blocks = 2); 131 072 + 259: 65 workgroups, eight trips; 1 048 576 + 2051: past the cap of 512 workgroups
SMALL_N = [1, 2, 3, 5, 255, 257, 2051]
LARGE_N = [131_072 + 259, 1_048_576 + 2051]
KS = [1, 3, 4, 5, 9]   # (f32 row groups hold 4 columns, f64 ones 2: one group, a padded one, a full one, a second, a third)
K_MAX = 9


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    """bit equality (any NaN equals any NaN: its sign and payload are not arithmetic)"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def raw(mv):
    """The interleaved storage as it is: (dim, ld)."""
    out = np.empty(mv.dim() * mv.ld(), mv.dtype)
    if out.size:
        _lib.check(sm.lib().smh_dev_download(out.ctypes.data, C.c_void_p(mv.data_ptr()), out.nbytes))
    return out.reshape(mv.dim(), mv.ld())


def matrix(off, col, val):
    n = len(off) - 1
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)


def solve_mvec(a, B, X0, tol, iter_max, check_every=0):
    b, x = sm.MultiVec.from_vecs(np.ascontiguousarray(B)), sm.MultiVec.from_vecs(np.ascontiguousarray(X0))
    s = sm.ConjugateGradient(tol, iter_max, check_every=check_every)
    assert s.solve_many(a, b, x) is x
    assert not bits(raw(x)[:, x.count():]).any(), "padding columns of x must hold +0"
    assert same(b.to_numpy(), np.ascontiguousarray(B))
    return x.to_numpy(), s.iterations, s.r_norm_squared


def solve_host(a, B, X0, tol, iter_max):
    x = np.array(X0, copy=True)
    s = sm.ConjugateGradient(tol, iter_max)
    assert s.solve_many(a, B, x) is x
    return x, s.iterations, s.r_norm_squared


def assert_columns(got, want, cols, what):
    """got: (x, iterations, r_norm_squared) of the device for len(cols) columns; want: a cg_many_model.Result; cols: which of
    its columns they are."""
    x, iters, rr = got
    assert isinstance(iters, np.ndarray) and iters.dtype.kind == "i" and iters.shape == (len(cols),), (what, iters)
    assert isinstance(rr, np.ndarray) and rr.dtype == np.float64 and rr.shape == (len(cols),), (what, rr)
    assert x.shape == (len(cols), want.x.shape[1]), (what, x.shape)
    for j, c in enumerate(cols):
        assert iters[j] == want.iterations[c], (what, "iterations of column", j, iters, want.iterations[list(cols)])
        assert same(rr[j], want.r_norm_squared[c]), (what, "r.r of column", j, rr[j], want.r_norm_squared[c])
        bad = np.flatnonzero(~((x[j] == want.x[c]) | (np.isnan(x[j]) & np.isnan(want.x[c]))))
        assert same(x[j], want.x[c]), (what, "x of column", j, len(bad), bad[:5], x[j][bad[:5]], want.x[c][bad[:5]])


@functools.lru_cache(maxsize=None)
def case(n, dtype_name, x0_random, tol, iter_max, k_max=K_MAX):
    """The tridiagonal system of n rows, k_max right-hand sides and starts, and the model's solve of every column (computed once,
    shared, read-only: a column of the model does not depend on which others are solved with it)."""
    dtype = np.dtype(dtype_name).type
    off, col, val = cg_model.tridiag(n, dtype, seed=n % 97)
    rng = np.random.default_rng(2000 + n)
    B = rng.uniform(-1, 1, (k_max, n)).astype(dtype)
    X0 = rng.uniform(-1, 1, (k_max, n)).astype(dtype) if x0_random else np.zeros((k_max, n), dtype)
    want = cg_many_model.cg_many(off, col, val, B, X0, tol, iter_max)
    for arr in (off, col, val, B, X0, want.x):
        arr.setflags(write=False)
    return off, col, val, B, X0, want


@functools.lru_cache(maxsize=None)
def handle(n, dtype_name):
    off, col, val = cg_model.tridiag(n, np.dtype(dtype_name).type, seed=n % 97)
    return matrix(off, col, val)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SMALL_N)
def test_bits_at_every_path_size(gpu, n, k, dtype):
    """tol 0, 6 bodies; check_every 2 (three replays of the captured batch), 7 (plain launches) and the default (4: two replays,
    the second half no-ops)."""
    name = np.dtype(dtype).name
    a = handle(n, name)
    for x0_random in (False, True):
        off, col, val, B, X0, want = case(n, name, x0_random, 0.0, 6)
        assert (want.iterations == 6).all()
        for check_every in (2, 7, 0):
            assert_columns(solve_mvec(a, B[:k], X0[:k], 0.0, 6, check_every), want, range(k), (n, k, x0_random, check_every))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", LARGE_N)
def test_bits_on_large_systems(gpu, n, dtype):
    """k = 2, 3 bodies: eight and nine trips per thread, the second size past the cap of 512 workgroups."""
    name = np.dtype(dtype).name
    off, col, val, B, X0, want = case(n, name, dtype == np.float32, 0.0, 3, 2)
    assert_columns(solve_mvec(handle(n, name), B, X0, 0.0, 3), want, range(2), n)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_on_a_non_banded_pattern(gpu, dtype):
    """laplace3d(7, 11, 13): n = 1001, seven entries per row, neighbours 1, 7 and 77 rows away."""
    off, col, val = oracle.laplace3d(7, 11, 13, dtype)
    n = 7 * 11 * 13
    a = matrix(off, col, val)
    rng = np.random.default_rng(5)
    B = rng.uniform(-1, 1, (5, n)).astype(dtype)
    for X0 in (np.zeros((5, n), dtype), rng.uniform(-1, 1, (5, n)).astype(dtype)):
        want = cg_many_model.cg_many(off, col, val, B, X0, 0.0, 10)
        assert_columns(solve_mvec(a, B, X0, 0.0, 10, 3), want, range(5), "laplace")
        assert_columns(solve_host(a, B, X0, 0.0, 10), want, range(5), "laplace host")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [257, 2051])
def test_columns_stop_in_different_bodies(gpu, n, dtype):
    """b_c = u_c * 10^-c, tol 1e-4, iter_max 40: the columns leave the loop one after the other, and a column frozen early keeps the
    x of its stopping body while its neighbours go on."""
    name = np.dtype(dtype).name
    off, col, val, U, _, _ = case(n, name, False, 0.0, 6)
    B = (U[:5] * (10.0 ** -np.arange(5))[:, None]).astype(dtype)
    X0 = np.zeros((5, n), dtype)
    want = cg_many_model.cg_many(off, col, val, B, X0, 1e-4, 40)
    assert len(set(want.iterations.tolist())) >= 3 and want.iterations.max() < 40, want.iterations   # (from the model)
    assert (np.sqrt(want.r_norm_squared) < 1e-4).all()
    a = handle(n, name)
    for check_every in (0, 3):
        got = solve_mvec(a, B, X0, 1e-4, 40, check_every)
        print("n = %d %s: bodies %s (model %s)" % (n, name, got[1].tolist(), want.iterations.tolist()))
        assert_columns(got, want, range(5), (n, check_every))
    # ... and in the opposite order of columns: the first to stop sits in another row group / at another place in its group
    got = solve_mvec(a, B[::-1], X0, 1e-4, 40)
    assert_columns(got, want, [4, 3, 2, 1, 0], (n, "reversed"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_iter_max_ends_the_loop_inside_a_replayed_batch(gpu, dtype):
    """iter_max 5 with check_every 4: the captured batch of four bodies runs twice, the last three bodies are no-ops."""
    name = np.dtype(dtype).name
    n = 257
    off, col, val, B, X0, _ = case(n, name, True, 0.0, 6)
    want = cg_many_model.cg_many(off, col, val, B[:5], X0[:5], 0.0, 5)
    assert (want.iterations == 5).all()
    assert_columns(solve_mvec(handle(n, name), B[:5], X0[:5], 0.0, 5, 4), want, range(5), "iter_max 5 / 4")
    # a tolerance that some columns meet and others do not, the rest ends on iter_max
    tol = float(np.sort(np.sqrt(want.r_norm_squared))[2]) * 1.0000001
    want = cg_many_model.cg_many(off, col, val, B[:5], X0[:5], tol, 5)
    assert_columns(solve_mvec(handle(n, name), B[:5], X0[:5], tol, 5, 4), want, range(5), "iter_max 5 / 4 with tol")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_nan_column_leaves_its_neighbours_alone(gpu, dtype):
    """b_c = 0 from x0 = 0: alpha = 0 / 0, the column fills with NaN and runs to iter_max like the reference; the other columns
    are bit for bit what they are without it."""
    name = np.dtype(dtype).name
    n = 2051
    off, col, val, B, X0, want = case(n, name, False, 0.0, 6)
    a = handle(n, name)
    for k, at in ((5, 2), (5, 4), (4, 0), (9, 5)):
        Bz = B[:k].copy()
        Bz[at] = 0
        x, iters, rr = solve_mvec(a, Bz, X0[:k], 0.0, 6)
        assert iters[at] == 6 and np.isnan(rr[at]) and np.isnan(x[at]).all(), (k, at)
        others = [c for c in range(k) if c != at]
        assert_columns((x[others], iters[others], rr[others]), want, others, ("beside NaN", k, at))
    # with a tolerance: the finite columns stop, the NaN column goes on to iter_max (sqrt(NaN) < tol is false)
    Bz = B[:5].copy()
    Bz[1] = 0
    want_t = cg_many_model.cg_many(off, col, val, Bz, X0[:5], 1e-3, 30)
    assert want_t.iterations[1] == 30 and want_t.iterations[[0, 2, 3, 4]].max() < 30
    assert_columns(solve_mvec(a, Bz, X0[:5], 1e-3, 30), want_t, range(5), "NaN column with tol")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_column_is_its_own_solve_wherever_it_stands(gpu, dtype):
    name = np.dtype(dtype).name
    n = 2051
    off, col, val, B, X0, want = case(n, name, True, 0.0, 6)
    a = handle(n, name)
    x5, it5, rr5 = solve_mvec(a, B[:5], X0[:5], 0.0, 6)
    for c in range(5):
        x1, it1, rr1 = solve_mvec(a, B[c:c + 1], X0[c:c + 1], 0.0, 6)
        assert same(x1[0], x5[c]) and it1[0] == it5[c] and same(rr1[0], rr5[c]), c
    perm = [3, 0, 4, 2, 1, 3, 8]
    xp, itp, rrp = solve_mvec(a, B[perm], X0[perm], 0.0, 6)
    for j, c in enumerate(perm):
        assert same(xp[j], want.x[c]) and itp[j] == want.iterations[c] and same(rrp[j], want.r_norm_squared[c]), (j, c)
    # two runs: equal bits
    xq, itq, rrq = solve_mvec(a, B[perm], X0[perm], 0.0, 6)
    assert same(xp, xq) and np.array_equal(itp, itq) and same(rrp, rrq)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_padding_stays_plus_zero_with_an_inf_in_the_matrix(gpu, dtype):
    """0 x Inf in the padding columns' products: X's padding columns, read raw, hold +0 afterwards (the data of X is NaN-free on
    entry; the solve itself goes non-finite)."""
    n = 259
    off, col, val = cg_model.tridiag(n, dtype, seed=2)
    val = val.copy()
    val[[4, 300]] = [np.inf, -np.inf]
    a = matrix(off, col, val)
    rng = np.random.default_rng(4)
    for k in (1, 3, 5):
        b = sm.MultiVec.from_vecs(rng.uniform(-1, 1, (k, n)).astype(dtype))
        x = sm.MultiVec.from_vecs(rng.uniform(-1, 1, (k, n)).astype(dtype))
        sm.ConjugateGradient(0.0, 5).solve_many(a, b, x)
        r = raw(x)
        assert r.shape == (n, x.ld()) and not bits(r[:, k:]).any(), k
        assert not np.isfinite(r[:, :k]).all()   # the case is what it claims to be


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_edges(gpu, dtype):
    # n = 0 against the model: tol 0 runs iter_max bodies on nothing; a tolerance stops in the first (r.r = +0)
    off, col, val = cg_model.tridiag(0, dtype)
    a = matrix(off, col, val)
    e = np.zeros((3, 0), dtype)
    for tol, iter_max in ((0.0, 5), (1e-6, 5), (0.0, 0)):
        want = cg_many_model.cg_many(off, col, val, e, e, tol, iter_max)
        assert_columns(solve_mvec(a, e, e, tol, iter_max), want, range(3), ("n = 0", tol, iter_max))
        assert_columns(solve_host(a, e, e, tol, iter_max), want, range(3), ("n = 0 host", tol, iter_max))
    assert cg_many_model.cg_many(off, col, val, e, e, 1e-6, 5).iterations.tolist() == [1, 1, 1]
    # iter_max = 0: the initial r.r, no body, x untouched
    name = np.dtype(dtype).name
    off, col, val, B, X0, _ = case(257, name, True, 0.0, 6)
    want = cg_many_model.cg_many(off, col, val, B[:3], X0[:3], 0.0, 0)
    got = solve_mvec(handle(257, name), B[:3], X0[:3], 0.0, 0)
    assert_columns(got, want, range(3), "iter_max = 0")
    assert got[1].tolist() == [0, 0, 0] and same(got[0], X0[:3]) and (got[2] > 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_entry_points_agree(gpu, dtype):
    name = np.dtype(dtype).name
    n = 2051
    off, col, val, B, X0, want = case(n, name, True, 0.0, 6)
    a = handle(n, name)
    for k in (1, 5):
        assert_columns(solve_host(a, B[:k], X0[:k], 0.0, 6), want, range(k), ("host", k))
        # array-likes for b; lists of rows
        x = X0[:k].copy()
        s = sm.ConjugateGradient(0.0, 6)
        s.solve_many(a, [row.tolist() for row in B[:k]], x)
        assert_columns((x, s.iterations, s.r_norm_squared), want, range(k), ("lists", k))
    with pytest.raises(TypeError):
        sm.ConjugateGradient().solve_many(a, B[:2], X0[:2].astype(np.float64 if dtype == np.float32 else np.float32))
    with pytest.raises(TypeError):
        sm.ConjugateGradient().solve_many(a, B[:2], X0[:2].copy().T)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_statuses(gpu, dtype):
    """Every status is decided on the host before any launch: x keeps what it held."""
    other = np.float64 if dtype == np.float32 else np.float32
    L = sm.lib()
    n = 40
    off, col, val = cg_model.tridiag(n, dtype, seed=1)
    a = matrix(off, col, val)
    sentinel = np.full((3, n), 7.0, dtype)
    x = sm.MultiVec.from_vecs(sentinel)
    b = sm.MultiVec.from_vecs(np.ones((3, n), dtype))
    iters = (C.c_size_t * 4)(9, 9, 9, 9)
    rr = (C.c_double * 4)(9.0, 9.0, 9.0, 9.0)

    def expect(rc, status, text):
        assert rc == status and text in L.smh_last_error().decode(), (rc, L.smh_last_error())
        assert np.array_equal(x.to_numpy(), sentinel) and list(iters) == [9] * 4 and list(rr) == [9.0] * 4   # nothing was launched

    def call(m, bb, xx, it=iters, r2=rr):
        return L.smh_cg_solve_many(m._h, bb._h if bb else None, xx._h if xx else None, 0.0, 5, 0, it, r2)

    rect = sm.SparseMatCRS.from_raw_parts(n, n + 1, off, col, val)
    expect(call(rect, b, x), _lib.SMH_ERR_NOT_SQUARE, "Matrix is not symmetric")
    expect(call(a, sm.MultiVec.zeros(n + 1, 3, dtype), x), _lib.SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch")
    expect(call(a, sm.MultiVec.zeros(n, 4, dtype), x), _lib.SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch")
    expect(call(a, sm.MultiVec.zeros(n, 3, other), x), _lib.SMH_ERR_INVALID, "dtype")
    expect(call(a, x, x), _lib.SMH_ERR_INVALID, "same storage")
    expect(call(a, b, x, None, rr), _lib.SMH_ERR_INVALID, "NULL output")
    expect(call(a, b, x, iters, None), _lib.SMH_ERR_INVALID, "NULL output")
    expect(call(a, None, x), _lib.SMH_ERR_INVALID, "NULL")
    xs = sm.MultiVec.from_vecs(np.full((3, n - 1), 7.0, dtype))
    assert call(a, b, xs) == _lib.SMH_ERR_DIM_MISMATCH and np.array_equal(xs.to_numpy(), np.full((3, n - 1), 7.0, dtype))
    x_other = sm.MultiVec.from_vecs(np.full((3, n), 7.0, other))
    assert call(a, b, x_other) == _lib.SMH_ERR_INVALID and np.array_equal(x_other.to_numpy(), np.full((3, n), 7.0, other))
    # K1m's own statuses pass through: a column index beyond the vectors' reach
    wide_col = col.copy()
    wide_col[5] = n + 3
    wide = sm.SparseMatCRS.from_raw_parts(n, n, off, wide_col, val, validate=False)
    expect(call(wide, b, x), _lib.SMH_ERR_INDEX_RANGE, "index out of bounds: the len is %d but the index is %d" % (n, n + 3))
    # the host entry
    xh = sentinel.copy()
    bh = np.ones((3, n), dtype)
    host = lambda m, nn, kk: L.smh_cg_solve_many_host(m._h, bh.ctypes.data, nn, kk, xh.ctypes.data, 0.0, 5, iters, rr)
    for rc, status in ((host(rect, n, 3), _lib.SMH_ERR_NOT_SQUARE), (host(a, n + 1, 3), _lib.SMH_ERR_DIM_MISMATCH), (host(a, n, 0), _lib.SMH_ERR_INVALID)):
        assert rc == status and np.array_equal(xh, sentinel) and list(iters) == [9] * 4
    # the Python mirror raises solve's panics
    with pytest.raises(sm.SparseMatPanic) as e:
        sm.ConjugateGradient().solve_many(rect, b, x)
    assert e.value.status == _lib.SMH_ERR_NOT_SQUARE and "Matrix is not symmetric" in str(e.value)
    with pytest.raises(sm.SparseMatPanic) as e:
        sm.ConjugateGradient().solve_many(a, np.ones((3, n + 1), dtype), np.zeros((3, n + 1), dtype))
    assert e.value.status == _lib.SMH_ERR_DIM_MISMATCH and "Matrix and vector size mismatch" in str(e.value)
    # and the call that all of these refused goes through
    assert call(a, b, x) == 0 and list(iters)[:3] == [5, 5, 5] and list(iters)[3] == 9
    want = cg_many_model.cg_many(off, col, val, np.ones((3, n), dtype), sentinel, 0.0, 5)
    assert same(x.to_numpy(), want.x) and same(np.array(list(rr)[:3]), want.r_norm_squared)
