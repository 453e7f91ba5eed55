"""K1m (the multi-vector product, spmv_many.hip) and MultiVec: every column BIT-EXACT against the oracle's storage-order sum
(sparsematrix.rs:146-158) and against the same handle's SEQ product, on the shapes of tests/test_stream_gpu.py, for k with and
without padding; the containers, the degenerate shapes, every status, non-finite data, determinism."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib, synth
from sparsemat_amd.multivec import leading_dim
from util import random_crs, value_class

pytestmark = pytest.mark.gpu
KINDS = ["short", "len8", "empty_heavy", "overflow_tile", "ragged"]
N_ROWS, N_COLS, K_MAX = 5003, 4001, 9


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def case(kind, dtype_name):
    """The matrix of one kind, K_MAX right-hand sides, the oracle's product of each and the handle's SEQ product of each."""
    dtype = np.dtype(dtype_name).type
    rng = np.random.default_rng({"short": 1, "len8": 2, "empty_heavy": 3, "overflow_tile": 4, "ragged": 5}[kind])
    if kind == "short":
        lens = rng.integers(0, 10, N_ROWS)
    elif kind == "len8":
        lens = np.full(N_ROWS, 8)  # a power-of-two stride in every plane of the stage
    elif kind == "empty_heavy":
        lens = rng.integers(0, 4, N_ROWS)
        lens[rng.random(N_ROWS) < 0.7] = 0
    elif kind == "overflow_tile":
        lens = rng.integers(0, 9, N_ROWS)
        lens[300:420] = 60  # tile 1 holds more entries than the stage
        lens[1000] = 5000   # a row that straddles passes
    else:
        lens = rng.integers(0, 40, N_ROWS)
    off, col, val = random_crs(rng, N_ROWS, N_COLS, lens, dtype, dup=True)
    X = rng.uniform(-1, 1, (K_MAX, N_COLS)).astype(dtype)
    Y = np.stack([oracle.spmv(off, col, val, X[c]) for c in range(K_MAX)])
    for a in (off, col, val, X, Y):
        a.setflags(write=False)
    return off, col, val, X, Y


@functools.lru_cache(maxsize=None)
def handle(kind, dtype_name):
    off, col, val, X, Y = case(kind, dtype_name)
    m = sm.SparseMatCRS.from_raw_parts(N_ROWS, N_COLS, off, col, val)
    seq = np.stack([m.mvp(X[c], variant="seq") for c in range(K_MAX)])
    return m, seq


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_mvp_many_bit_exact(gpu, kind, dtype, k):
    off, col, val, X, Y = case(kind, np.dtype(dtype).name)
    m, seq = handle(kind, np.dtype(dtype).name)
    mv = sm.MultiVec.from_vecs(X[:k])
    assert (mv.dim(), mv.count(), mv.ld()) == (N_COLS, k, leading_dim(k))
    out = m.mvp_many(mv)
    assert isinstance(out, sm.MultiVec) and (out.dim(), out.count(), out.dtype) == (N_ROWS, k, np.dtype(dtype))
    y = out.to_numpy()
    assert y.shape == (k, N_ROWS)
    for c in range(k):
        assert np.array_equal(bits(y[c]), bits(Y[c])), "%s k=%d column %d: %d rows differ from the oracle" % (kind, k, c, (bits(y[c]) != bits(Y[c])).sum())
        assert np.array_equal(bits(y[c]), bits(seq[c])), "%s k=%d column %d differs from SEQ" % (kind, k, c)


def test_mvp_many_on_laplacians_and_borrowed_unpadded_arrays(gpu):
    rng = np.random.default_rng(11)
    for dims in [(37, 23, 1), (9, 7, 5), (64, 64, 4)]:
        off, col, val = oracle.laplace3d(*dims, np.float32)
        n = dims[0] * dims[1] * dims[2]
        X = np.stack([oracle.gen_x(synth.SEED_X, n, np.float32)] + [rng.uniform(-1, 1, n).astype(np.float32) for _ in range(4)])
        m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
        y = m.mvp_many(X)
        for c in range(5):
            assert np.array_equal(bits(y[c]), bits(oracle.spmv(off, col, val, X[c]))), (dims, c)
    # device-born Laplacian: borrowed arrays whose nnz is not a multiple of 4 (tail chunk read entry by entry)
    row_end = next(re for re in range(300, 310) if synth.laplace3d_nnz(11, 7, 5, 13, re) % 4 != 0)
    m = synth.crs_laplace3d(11, 7, 5, np.float32, 13, row_end)
    off, col, val = m.raw_parts()
    assert len(val) % 4 != 0
    for k in (3, 8):
        X = np.stack([oracle.gen_x(synth.SEED_X, 11 * 7 * 5, np.float32)] + [rng.uniform(-1, 1, 11 * 7 * 5).astype(np.float32) for _ in range(k - 1)])
        y = m.mvp_many(sm.MultiVec.from_vecs(X)).to_numpy()
        for c in range(k):
            assert np.array_equal(bits(y[c]), bits(oracle.spmv(off, col, val, X[c]))), (k, c)


def raw(mv):
    """The interleaved storage as it is: (dim, ld)."""
    out = np.empty(mv.dim() * mv.ld(), mv.dtype)
    _lib.check(sm.lib().smh_dev_download(out.ctypes.data, C.c_void_p(mv.data_ptr()), out.nbytes))
    return out.reshape(mv.dim(), mv.ld())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_containers(gpu, dtype):
    rng = np.random.default_rng(12)
    for k, n in [(1, 1), (3, 63), (4, 64), (5, 65), (9, 1000), (33, 130), (2, 0)]:   # tiles of 64 x 32: partial ones, more than one of each
        a = rng.uniform(-1, 1, (k, n)).astype(dtype)
        mv = sm.MultiVec.from_vecs(a)
        assert (mv.dim(), mv.count(), mv.ld(), mv.dtype) == (n, k, leading_dim(k), np.dtype(dtype))
        assert np.array_equal(bits(mv.to_numpy()), bits(a))
        if n:
            r = raw(mv)
            assert np.array_equal(bits(r[:, :k]), bits(a.T)) and not bits(r[:, k:]).any()   # element i of vector c at [i * ld + c]; padding +0
        # column <-> DenseVec
        for c in {0, k // 2, k - 1}:
            assert np.array_equal(bits(mv.column(c).to_numpy()), bits(a[c]))
        v = rng.uniform(-1, 1, n).astype(dtype)
        mv.set_column(k - 1, sm.DenseVec.from_vec(v))
        a[k - 1] = v
        mv.set_column(0, a[0][::-1].copy())   # an array-like goes through a DenseVec
        a[0] = a[0][::-1].copy()
        assert np.array_equal(bits(mv.to_numpy()), bits(a)) and (n == 0 or not bits(raw(mv)[:, k:]).any())
        # from DenseVecs (device to device) and from a list of arrays
        assert np.array_equal(bits(sm.MultiVec.from_vecs([sm.DenseVec.from_vec(row) for row in a]).to_numpy()), bits(a))
        assert np.array_equal(bits(sm.MultiVec.from_vecs([row for row in a]).to_numpy()), bits(a))
    z = sm.MultiVec.zeros(70, 5, dtype)
    assert not bits(raw(z)).any() and z.to_numpy().shape == (5, 70)
    # column statuses
    mv = sm.MultiVec.zeros(10, 3, dtype)
    other = np.float64 if dtype == np.float32 else np.float32
    for fn, status, text in [(lambda: mv.column(3), _lib.SMH_ERR_INVALID, "column 3"),
                             (lambda: mv.set_column(3, sm.DenseVec.zeros(10, dtype)), _lib.SMH_ERR_INVALID, "column 3"),
                             (lambda: mv.set_column(0, sm.DenseVec.zeros(11, dtype)), _lib.SMH_ERR_DIM_MISMATCH, "Dimension mismatch"),
                             (lambda: mv.set_column(0, sm.DenseVec.zeros(10, other)), _lib.SMH_ERR_INVALID, "dtype mismatch")]:
        with pytest.raises(sm.SparseMatPanic) as e:
            fn()
        assert e.value.status == status and text in str(e.value)
    v = sm.DenseVec.zeros(9, dtype)
    assert sm.lib().smh_mvec_get_column(mv._h, 0, v._h) == _lib.SMH_ERR_DIM_MISMATCH


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_padding_columns_stay_zero_and_the_three_entries_agree(gpu, dtype):
    off, col, val, X, Y = case("ragged", np.dtype(dtype).name)
    k = 5
    for with_inf in (False, True):
        v = val.copy()
        if with_inf:
            v[[3, 700, 9000]] = [np.inf, -np.inf, np.inf]   # 0 x Inf in the padding columns' products
        m = sm.SparseMatCRS.from_raw_parts(N_ROWS, N_COLS, off, col, v)
        x = sm.MultiVec.from_vecs(X[:k])
        out = m.mvp_many(x)
        r = raw(out)
        assert r.shape == (N_ROWS, 8) and not bits(r[:, k:]).any(), "padding columns of y must hold +0"
        y = out.to_numpy()
        with np.errstate(invalid="ignore", over="ignore"):
            want = np.stack([oracle.spmv(off, col, v, X[c]) for c in range(k)])
        fin = np.isfinite(want)
        assert np.array_equal(value_class(y), value_class(want)) and np.array_equal(bits(y)[fin], bits(want)[fin])
        # the host-pointer entry and the raw device entry: the same bits (y pre-filled with NaN, padding included: all overwritten)
        y_host = m.mvp_many(X[:k])
        assert isinstance(y_host, np.ndarray) and y_host.shape == (k, N_ROWS) and np.array_equal(bits(y_host), bits(y))
        ybuf = synth.DeviceBuffer(N_ROWS * 8 * y.itemsize)
        ybuf.upload(np.full(N_ROWS * 8, np.nan, dtype))
        m.mvp_many_dev(x.data_ptr(), N_COLS, ybuf.ptr, k, 8)
        _lib.check(sm.lib().smh_device_synchronize())
        assert np.array_equal(bits(ybuf.download(dtype, N_ROWS * 8).reshape(N_ROWS, 8)), bits(r))


def test_degenerate_shapes(gpu):
    f = np.float32
    X = np.arange(6, dtype=f).reshape(2, 3) + 1
    # no rows
    m = sm.SparseMatCRS.from_raw_parts(0, 3, [0], [], np.array([], f))
    assert m.mvp_many(X).shape == (2, 0)
    out = m.mvp_many(sm.MultiVec.from_vecs(X))
    assert (out.dim(), out.count()) == (0, 2) and out.to_numpy().shape == (2, 0)
    # rows without entries: zeros (+0), also over stale storage
    m = sm.SparseMatCRS.from_raw_parts(5, 3, [0, 0, 0, 0, 0, 0], [], np.array([], f))
    assert np.array_equal(bits(m.mvp_many(X)), bits(np.zeros((2, 5), f)))
    assert not bits(m.mvp_many(sm.MultiVec.from_vecs(X)).to_numpy()).any()
    # a single row; x.dim() > n_cols
    m = sm.SparseMatCRS.from_raw_parts(1, 2, [0, 2], [1, 0], np.array([2.5, -1.0], f))
    Xl = np.array([[1, 3, 9], [2, -4, 7], [0, 1, 5]], f)
    assert np.array_equal(m.mvp_many(Xl), np.array([[6.5], [-12.0], [2.5]], f))
    assert np.array_equal(m.mvp_many(sm.MultiVec.from_vecs(Xl)).to_numpy(), np.array([[6.5], [-12.0], [2.5]], f))
    # k = 1 is the single product, bit for bit; tile boundaries
    rng = np.random.default_rng(8)
    for n_rows in (255, 256, 257, 513):
        off, col, val = random_crs(rng, n_rows, 100, rng.integers(0, 7, n_rows), f)
        x = rng.uniform(-1, 1, 100).astype(f)
        m = sm.SparseMatCRS.from_raw_parts(n_rows, 100, off, col, val)
        y1 = m.mvp_many(x[None, :])
        assert y1.shape == (1, n_rows) and np.array_equal(bits(y1[0]), bits(m.mvp(x, variant="stream")))
        assert np.array_equal(bits(y1[0]), bits(oracle.spmv(off, col, val, x)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_statuses(gpu, dtype):
    """Every status is decided on the host before any launch: y keeps what it held."""
    other = np.float64 if dtype == np.float32 else np.float32
    rng = np.random.default_rng(3)
    off, col, val = random_crs(rng, 40, 30, rng.integers(1, 5, 40), dtype)
    col[0] = 29   # max_col = 29
    m = sm.SparseMatCRS.from_raw_parts(40, 30, off, col, val)
    L = sm.lib()
    x = sm.MultiVec.from_vecs(rng.uniform(-1, 1, (3, 30)).astype(dtype))
    sentinel = np.full((3, 40), 7.0, dtype)
    y = sm.MultiVec.from_vecs(sentinel)

    def expect(rc, status, text):
        assert rc == status and text in L.smh_last_error().decode(), (rc, L.smh_last_error())
        assert np.array_equal(y.to_numpy(), sentinel)   # nothing was launched

    x_other, y_other = sm.MultiVec.zeros(30, 3, other), sm.MultiVec.zeros(40, 3, other)
    y_rows, y_count, x_short = sm.MultiVec.zeros(41, 3, dtype), sm.MultiVec.zeros(40, 4, dtype), sm.MultiVec.zeros(29, 3, dtype)
    expect(L.smh_crs_spmv_many(m._h, x._h, x._h), _lib.SMH_ERR_INVALID, "same storage")                     # x is y
    expect(L.smh_crs_spmv_many(m._h, x_other._h, y._h), _lib.SMH_ERR_INVALID, "dtype")
    expect(L.smh_crs_spmv_many(m._h, x._h, y_other._h), _lib.SMH_ERR_INVALID, "dtype")
    expect(L.smh_crs_spmv_many(m._h, x._h, y_rows._h), _lib.SMH_ERR_DIM_MISMATCH, "Dimension mismatch")
    expect(L.smh_crs_spmv_many(m._h, x._h, y_count._h), _lib.SMH_ERR_DIM_MISMATCH, "Dimension mismatch")
    expect(L.smh_crs_spmv_many(m._h, x_short._h, y._h), _lib.SMH_ERR_INDEX_RANGE, "index out of bounds: the len is 29 but the index is 29")
    with pytest.raises(sm.SparseMatPanic) as e:   # ... and through the Python mirror
        m.mvp_many(x_short)
    assert e.value.status == _lib.SMH_ERR_INDEX_RANGE
    with pytest.raises(sm.SparseMatPanic) as e:   # ... through the host-pointer entry, with mvp's wording
        m.mvp_many(np.zeros((2, 29), dtype))
    assert e.value.status == _lib.SMH_ERR_INDEX_RANGE and "index out of bounds: the len is 29 but the index is 29" in str(e.value)
    with pytest.raises(sm.SparseMatPanic) as e:
        m.mvp(np.zeros(29, dtype))
    assert "index out of bounds: the len is 29 but the index is 29" in str(e.value)
    # the raw device entry
    xp, yp, s = x.data_ptr(), y.data_ptr(), np.dtype(dtype).itemsize
    dev = lambda xq, x_len, yq, k, ld: L.smh_crs_spmv_many_dev(m._h, C.c_void_p(xq), x_len, C.c_void_p(yq), k, ld, None)
    expect(dev(xp, 30, yp, 0, 4), _lib.SMH_ERR_INVALID, "k == 0")
    expect(dev(xp, 30, xp, 3, 4), _lib.SMH_ERR_INVALID, "same storage")
    expect(dev(xp + s, 30, yp, 3, 4), _lib.SMH_ERR_INVALID, "16-byte aligned")
    expect(dev(xp, 30, yp + s, 3, 4), _lib.SMH_ERR_INVALID, "16-byte aligned")
    expect(dev(xp, 30, yp, 3, 3), _lib.SMH_ERR_INVALID, "multiple of 4")
    expect(dev(xp, 30, yp, 5, 4), _lib.SMH_ERR_INVALID, "at least k")
    expect(dev(xp, (1 << 62), yp, 3, 4), _lib.SMH_ERR_INVALID, "address space")   # n * ld * sizeof(T) overflows
    expect(dev(xp, 29, yp, 3, 4), _lib.SMH_ERR_INDEX_RANGE, "index out of bounds: the len is 29 but the index is 29")
    expect(dev(0, 30, yp, 3, 4), _lib.SMH_ERR_INVALID, "NULL")
    expect(L.smh_crs_spmv_many_host(m._h, None, 30, 0, None), _lib.SMH_ERR_INVALID, "k == 0")
    h = C.c_void_p()
    expect(L.smh_mvec_create(_lib.dtype_code(dtype), 5, 0, C.byref(h)), _lib.SMH_ERR_INVALID, "k == 0")
    # and the call that all of these refused goes through
    assert L.smh_crs_spmv_many(m._h, x._h, y._h) == 0
    assert np.array_equal(bits(y.to_numpy()), bits(np.stack([oracle.spmv(off, col, val, xc) for xc in x.to_numpy()])))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_non_finite_data(gpu, dtype):
    """NaN, +-Inf and +-0 in some stored values and in some entries of SOME columns of X: rows in which the oracle is non-finite
    are compared by class, all others bit for bit; a column whose own data is finite is the oracle's bit for bit -- a
    neighbour's NaN does not cross over."""
    off, col, val, X, _ = case("ragged", np.dtype(dtype).name)
    k = 5
    rng = np.random.default_rng(66)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype)
    X = X[:k].copy()
    for c in (1, 3, 4):   # columns 0 and 2 keep finite data (4 sits beside the padding)
        at = rng.choice(N_COLS, 60, replace=False)
        X[c, at] = specials[rng.integers(0, 5, 60)]
    for values in (val, None):
        v = val.copy()
        if values is None:   # ... and in the matrix: only zeros of both signs first (columns 0 and 2 stay finite), then everything
            at = rng.choice(len(v), 200, replace=False)
            v[at] = specials[rng.integers(0, 5, 200)]
        else:
            at = rng.choice(len(v), 200, replace=False)
            v[at] = specials[3 + rng.integers(0, 2, 200)]
        m = sm.SparseMatCRS.from_raw_parts(N_ROWS, N_COLS, off, col, v)
        with np.errstate(invalid="ignore", over="ignore"):
            want = np.stack([oracle.spmv(off, col, v, X[c]) for c in range(k)])
        for y in (m.mvp_many(sm.MultiVec.from_vecs(X)).to_numpy(), m.mvp_many(X)):
            cls = value_class(want)
            assert np.array_equal(value_class(y), cls)
            assert np.array_equal(bits(y)[cls == 0], bits(want)[cls == 0])
            if values is not None:
                assert (cls[[1, 3, 4]] != 0).any() and not cls[[0, 2]].any()   # the case is what it claims to be
                for c in (0, 2):
                    assert np.array_equal(bits(y[c]), bits(want[c]))
            else:
                assert (cls[[0, 2]] != 0).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_determinism(gpu, dtype):
    off, col, val, X, Y = case("overflow_tile", np.dtype(dtype).name)
    m, _ = handle("overflow_tile", np.dtype(dtype).name)
    x = sm.MultiVec.from_vecs(X[:7])
    a, b = m.mvp_many(x), m.mvp_many(x)
    assert np.array_equal(bits(a.to_numpy()), bits(b.to_numpy())) and np.array_equal(bits(a.to_numpy()), bits(Y[:7]))
    assert np.array_equal(bits(m.mvp_many(X[:7])), bits(m.mvp_many(X[:7])))
