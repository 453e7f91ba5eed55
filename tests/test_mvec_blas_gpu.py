"""The per-column BLAS-1 of MultiVec (mvec_blas.hip): add / sub / scale / copy bit for bit against numpy with one rounding per
operation; dot / norm_squared bit for bit against the column tree (cg_many_model.column_sum), whose order depends on n alone;
padding columns read raw: +0 after every operation; every status."""
import ctypes as C
import functools

import numpy as np
import pytest

import cg_many_model
import sparsemat_amd as sm
from sparsemat_amd import _lib
from sparsemat_amd.multivec import leading_dim

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
SMALL_N = [0, 1, 3, 255, 257, 2051]
LARGE_N = [131_072 + 259, 1_048_576 + 2051]   # 65 workgroups, eight trips per thread; 514 -> the cap of 512: a ninth trip
KS = [1, 3, 4, 5, 8]
K_MAX = 8


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def raw(mv):
    """The interleaved storage as it is: (dim, ld)."""
    out = np.empty(mv.dim() * mv.ld(), mv.dtype)
    if out.size:
        _lib.check(sm.lib().smh_dev_download(out.ctypes.data, C.c_void_p(mv.data_ptr()), out.nbytes))
    return out.reshape(mv.dim(), mv.ld())


def padding_is_plus_zero(mv):
    return not bits(raw(mv)[:, mv.count():]).any()


@functools.lru_cache(maxsize=None)
def data(n, dtype_name, k_max=K_MAX):
    """k_max columns of x and y, and the tree's x_c . y_c and x_c . x_c of each (computed once, shared, read-only)."""
    dtype = np.dtype(dtype_name).type
    rng = np.random.default_rng(n + 5)
    X = rng.uniform(-1, 1, (k_max, n)).astype(dtype)
    Y = rng.uniform(-1, 1, (k_max, n)).astype(dtype)
    dot = np.array([cg_many_model.column_sum(X[c] * Y[c]) for c in range(k_max)], dtype)
    nsq = np.array([cg_many_model.column_sum(X[c] * X[c]) for c in range(k_max)], dtype)
    for a in (X, Y, dot, nsq):
        a.setflags(write=False)
    return X, Y, dot, nsq


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SMALL_N)
def test_elementwise_and_reductions_bit_exact(gpu, n, k, dtype):
    X, Y, dot, nsq = data(n, np.dtype(dtype).name)
    X, Y = X[:k], Y[:k]
    x, y = sm.MultiVec.from_vecs(X.copy()), sm.MultiVec.from_vecs(Y.copy())
    assert (x.dim(), x.count(), x.ld()) == (n, k, leading_dim(k))
    # reductions: f64 arrays of k, the tree's bits
    d, q = x.dot(y), x.norm_squared()
    assert d.dtype == np.float64 and d.shape == (k,) and q.shape == (k,)
    assert np.array_equal(d, dot[:k].astype(np.float64)), (d, dot[:k])
    assert np.array_equal(q, nsq[:k].astype(np.float64)), (q, nsq[:k])
    # copy / add / sub / scale: one rounding per operation
    z = x.copy()
    assert z is not x and z.data_ptr() != x.data_ptr() and np.array_equal(bits(z.to_numpy()), bits(X)) and padding_is_plus_zero(z)
    assert z.add(y) is z
    assert np.array_equal(bits(z.to_numpy()), bits(X + Y)) and padding_is_plus_zero(z)
    z.sub(y).sub(y)
    assert np.array_equal(bits(z.to_numpy()), bits((X + Y) - Y - Y)) and padding_is_plus_zero(z)
    f = np.array([1.5, -0.3, 1e-3, 7.0, 0.1, -2.0, 3.0, 0.7])[:k]
    z.scale(f)
    want = ((X + Y) - Y - Y) * f.astype(dtype)[:, None]   # T(a[c]), then one multiplication in T
    assert want.dtype == dtype and np.array_equal(bits(z.to_numpy()), bits(want)) and padding_is_plus_zero(z)
    # the operands are untouched
    assert np.array_equal(bits(x.to_numpy()), bits(X)) and np.array_equal(bits(y.to_numpy()), bits(Y))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", LARGE_N)
def test_reductions_on_large_vectors(gpu, n, dtype):
    """More than one trip per thread, and past the cap of 512 workgroups; k = 2."""
    X, Y, dot, nsq = data(n, np.dtype(dtype).name, 2)
    x, y = sm.MultiVec.from_vecs(X), sm.MultiVec.from_vecs(Y)
    assert np.array_equal(x.dot(y), dot.astype(np.float64))
    assert np.array_equal(x.norm_squared(), nsq.astype(np.float64))
    x.add(y)
    assert np.array_equal(bits(x.to_numpy()), bits(X + Y)) and padding_is_plus_zero(x)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_column_does_not_depend_on_its_neighbours_or_its_position(gpu, dtype):
    X, Y, dot, _ = data(2051, np.dtype(dtype).name)
    for pick in ([3], [7, 3, 0], [0, 1, 2, 3, 3], [5, 4, 3, 2, 1, 0, 6, 7, 3]):
        got = sm.MultiVec.from_vecs(X[pick]).dot(sm.MultiVec.from_vecs(Y[pick]))
        assert np.array_equal(got, dot[pick].astype(np.float64)), pick
    # a NaN column beside finite ones
    Xn = X[:3].copy()
    Xn[1, 100] = np.nan
    got = sm.MultiVec.from_vecs(Xn).dot(sm.MultiVec.from_vecs(Y[:3]))
    assert np.isnan(got[1]) and np.array_equal(got[[0, 2]], dot[[0, 2]].astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [1, 3, 5])
def test_padding_columns_stay_plus_zero(gpu, k, dtype):
    """... after every operation, also scale by +-Inf and NaN, and with non-finite data in the columns."""
    n = 259
    X, Y, _, _ = data(n, np.dtype(dtype).name)
    X, Y = X[:k].copy(), Y[:k].copy()
    X[0, 5], Y[k - 1, 7] = np.inf, np.nan
    x, y = sm.MultiVec.from_vecs(X), sm.MultiVec.from_vecs(Y)
    assert padding_is_plus_zero(x) and padding_is_plus_zero(y)
    for factors in (np.full(k, np.inf), np.full(k, -np.inf), np.full(k, np.nan), np.full(k, -1.0), np.full(k, -0.0)):
        z = sm.MultiVec.from_vecs(Y[::-1].copy())
        z.scale(factors)
        assert padding_is_plus_zero(z), factors
        with np.errstate(invalid="ignore"):
            want = Y[::-1] * factors.astype(dtype)[:, None]
        got = z.to_numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])
    x.add(y)
    assert padding_is_plus_zero(x)
    x.sub(y)
    assert padding_is_plus_zero(x)
    x.sub(x)   # x - x: +0 where finite
    assert padding_is_plus_zero(x)
    c = x.copy()
    assert padding_is_plus_zero(c)
    x.dot(y), x.norm_squared()
    assert padding_is_plus_zero(x) and padding_is_plus_zero(y)
    one = sm.MultiVec.from_vecs(np.ones((k, n), dtype))
    one.scale(2.0)   # a scalar scales every column
    assert np.array_equal(one.to_numpy(), np.full((k, n), 2.0, dtype)) and padding_is_plus_zero(one)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_statuses(gpu, dtype):
    """Every status is decided on the host before any launch: the operands keep what they held."""
    other = np.float64 if dtype == np.float32 else np.float32
    L = sm.lib()
    sentinel = np.full((3, 40), 7.0, dtype)
    x = sm.MultiVec.from_vecs(sentinel)
    y = sm.MultiVec.from_vecs(np.full((3, 40), 2.0, dtype))
    y_dim, y_count, y_other = sm.MultiVec.zeros(41, 3, dtype), sm.MultiVec.zeros(40, 4, dtype), sm.MultiVec.zeros(40, 3, other)
    out = (C.c_double * 4)(9.0, 9.0, 9.0, 9.0)
    fac = (C.c_double * 3)(2.0, 2.0, 2.0)

    def expect(rc, status, text):
        assert rc == status and text in L.smh_last_error().decode(), (rc, L.smh_last_error())
        assert np.array_equal(x.to_numpy(), sentinel) and list(out) == [9.0] * 4   # nothing was launched

    for fn in (L.smh_mvec_copy, L.smh_mvec_add, L.smh_mvec_sub):
        expect(fn(x._h, y_dim._h), _lib.SMH_ERR_DIM_MISMATCH, "Dimension mismatch")
        expect(fn(x._h, y_count._h), _lib.SMH_ERR_DIM_MISMATCH, "Dimension mismatch")
        expect(fn(x._h, y_other._h), _lib.SMH_ERR_INVALID, "dtype")
        expect(fn(x._h, None), _lib.SMH_ERR_INVALID, "NULL")
        expect(fn(None, y._h), _lib.SMH_ERR_INVALID, "NULL")
    expect(L.smh_mvec_dot(x._h, y_dim._h, out), _lib.SMH_ERR_DIM_MISMATCH, "Dimension mismatch")
    expect(L.smh_mvec_dot(x._h, y_count._h, out), _lib.SMH_ERR_DIM_MISMATCH, "Dimension mismatch")
    expect(L.smh_mvec_dot(x._h, y_other._h, out), _lib.SMH_ERR_INVALID, "dtype")
    expect(L.smh_mvec_dot(x._h, y._h, None), _lib.SMH_ERR_INVALID, "NULL output")
    expect(L.smh_mvec_norm_squared(x._h, None), _lib.SMH_ERR_INVALID, "NULL output")
    expect(L.smh_mvec_norm_squared(None, out), _lib.SMH_ERR_INVALID, "NULL")
    expect(L.smh_mvec_scale(x._h, None), _lib.SMH_ERR_INVALID, "NULL factor")
    expect(L.smh_mvec_scale(None, fac), _lib.SMH_ERR_INVALID, "NULL")
    with pytest.raises(sm.SparseMatPanic) as e:   # ... and through the Python mirror
        x.add(y_dim)
    assert e.value.status == _lib.SMH_ERR_DIM_MISMATCH
    with pytest.raises(sm.SparseMatPanic) as e:
        x.dot(y_other)
    assert e.value.status == _lib.SMH_ERR_INVALID
    # and the calls that all of these refused go through
    assert L.smh_mvec_dot(x._h, y._h, out) == 0 and list(out) == [560.0, 560.0, 560.0, 9.0]
    assert L.smh_mvec_scale(x._h, fac) == 0 and np.array_equal(x.to_numpy(), 2 * sentinel)
    # x with itself: allowed (x += x, x . x)
    assert L.smh_mvec_add(x._h, x._h) == 0 and np.array_equal(x.to_numpy(), 4 * sentinel)
    assert L.smh_mvec_copy(x._h, x._h) == 0 and np.array_equal(x.to_numpy(), 4 * sentinel)
