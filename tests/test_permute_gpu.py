"""GPU: row / column permutation of a CRS matrix, permutation of a vector and the bandwidth query (csrc/permute.hip), bit for
bit against their numpy restatement (tests/reorder_model.py); the statuses of malformed permutations; and the product
identity B x[p] == (A x)[p] for B = P A P^T through the storage-order kernels.

The emit kernel takes tiles of 1024 output entries and stages the offsets of up to 1024 rows per tile in LDS
(kPermTile, kPermStageRows in permute.hip); MIXED below has rows shorter and longer than a tile, rows ending on both sides of
a tile boundary and a run of empty rows longer than the stage."""
import ctypes as C

import numpy as np
import pytest

import reorder_model as rm
import sparsemat_amd as sm
from sparsemat_amd import _lib
import util

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
# lengths 0, 1, 63, 64, 65, 300, 5000; 1500 empty rows inside one tile (more rows than the LDS stage holds); a row that ends
# exactly on the tile boundary 8192 and one that starts there and fills a whole tile; many short rows
_HEAD = [0, 1, 63, 64, 65, 300, 5000] + [2] + [0] * 1500 + [7] + [0, 3, 1] * 400
MIXED_LENGTHS = _HEAD + [8192 - sum(_HEAD), 1024, 1023, 1025] + [5] * 300 + [0, 0]
MIXED_COLS = 777


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _mixed(dtype, seed=5):
    rng = np.random.default_rng(seed)
    n_rows = len(MIXED_LENGTHS)
    off, col, val = util.random_crs(rng, n_rows, MIXED_COLS, MIXED_LENGTHS, dtype, dup=True)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], dtype)
    val[rng.integers(0, len(val), 64)] = special[rng.integers(0, len(special), 64)]
    val[:5] = special
    assert off[len(_HEAD) + 1] == 8192 and off[-1] > 12 * 1024
    return n_rows, MIXED_COLS, off, col, val


def _same(mat, arrays, n_rows, n_cols):
    o, c, v = mat.raw_parts()
    assert mat.n_rows() == n_rows and mat.n_cols() == n_cols
    assert (o == arrays[0]).all()
    assert (c == arrays[1]).all()
    assert (_bits(v) == _bits(arrays[2])).all()


@pytest.fixture(scope="module", params=DTYPES, ids=["f32", "f64"])
def mixed(request, gpu):
    n_rows, n_cols, off, col, val = _mixed(request.param)
    for a in (off, col, val):
        a.setflags(write=False)
    return n_rows, n_cols, off, col, val, sm.SparseMatCRS.from_raw_parts(n_rows, n_cols, off, col, val)


@pytest.mark.parametrize("form", ["rows", "cols", "both"])
def test_permute_rectangular_matches_the_model(mixed, form):
    n_rows, n_cols, off, col, val, A = mixed
    rng = np.random.default_rng(17)
    rp = rng.permutation(n_rows).astype(np.uint32) if form != "cols" else None
    cp = rng.permutation(n_cols).astype(np.uint32) if form != "rows" else None
    B = A.permute(rp, cp)
    _same(B, rm.permute(n_rows, n_cols, off, col, val, rp, cp), n_rows, n_cols)
    _same(A, (off, col, val), n_rows, n_cols)
    assert B.max_row_len() == 5000


def test_identity_is_a_bitwise_copy_and_the_inverse_undoes(mixed):
    n_rows, n_cols, off, col, val, A = mixed
    _same(A.permute(), (off, col, val), n_rows, n_cols)
    _same(A.permute(np.arange(n_rows), np.arange(n_cols)), (off, col, val), n_rows, n_cols)
    rng = np.random.default_rng(23)
    rp, cp = rng.permutation(n_rows).astype(np.uint32), rng.permutation(n_cols).astype(np.uint32)
    back = A.permute(rp, cp).permute(rm.inverse(rp), rm.inverse(cp))
    _same(back, (off, col, val), n_rows, n_cols)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_permute_symmetric_and_bandwidth(gpu, dtype):
    rng = np.random.default_rng(29)
    n = 1500
    off, col, val = util.random_crs(rng, n, n, rng.integers(0, 40, n), dtype, dup=True)
    A = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    assert A.bandwidth() == rm.bandwidth(n, off, col)
    p = rng.permutation(n).astype(np.uint32)
    want = rm.permute_symmetric(n, off, col, val, p)
    B = A.permute_symmetric(p)
    _same(B, want, n, n)
    assert B.bandwidth() == rm.bandwidth(n, want[0], want[1])
    # a lower-triangular band: upper bandwidth 0
    _, o, c, v = rm.from_edges(50, np.arange(7, 50), np.arange(0, 43), dtype)
    assert sm.SparseMatCRS.from_raw_parts(50, 50, o, c, v).bandwidth() == (7, 0)
    assert sm.SparseMatCRS.from_raw_parts(4, 4, [0, 0, 0, 0, 0], [], np.zeros(0, dtype)).bandwidth() == (0, 0)


def test_empty_shapes(gpu):
    E = sm.SparseMatCRS.from_raw_parts(3, 5, [0, 0, 0, 0], [], np.zeros(0, np.float32))
    B = E.permute([2, 0, 1], [4, 3, 2, 1, 0])
    assert B.n_rows() == 3 and B.n_cols() == 5 and B.n_non_zero_entries() == 0 and (B.raw_parts()[0] == 0).all()
    Z = sm.SparseMatCRS.from_raw_parts(0, 0, [0], [], np.zeros(0, np.float64))
    assert Z.permute_symmetric([]).n_rows() == 0


def _raw_permute(A, rp, cp):
    """straight through the C ABI: (status, message, handle value)"""
    h = C.c_void_p(12345)
    r = None if rp is None else np.ascontiguousarray(rp, np.uint32)
    c = None if cp is None else np.ascontiguousarray(cp, np.uint32)
    rc = sm.lib().smh_crs_permute(A._h, None if r is None else r.ctypes.data, 0 if r is None else len(r),
                                  None if c is None else c.ctypes.data, 0 if c is None else len(c), C.byref(h))
    return rc, sm.lib().smh_last_error().decode(), h.value


def test_malformed_permutations_are_refused_and_leave_everything_untouched(mixed):
    n_rows, n_cols, off, col, val, A = mixed
    good_r, good_c = np.arange(n_rows, dtype=np.uint32), np.arange(n_cols, dtype=np.uint32)
    # wrong length
    rc, msg, h = _raw_permute(A, good_r[:-1], None)
    assert rc == _lib.SMH_ERR_DIM_MISMATCH and "row_perm has %d entries, %d expected" % (n_rows - 1, n_rows) in msg and h is None
    rc, msg, h = _raw_permute(A, None, np.append(good_c, 0))
    assert rc == _lib.SMH_ERR_DIM_MISMATCH and "col_perm has %d entries" % (n_cols + 1) in msg and h is None
    # an entry >= n: the FIRST offending position is named
    bad = good_r.copy()
    bad[[900, 40]] = [n_rows, 4000000000]
    rc, msg, h = _raw_permute(A, bad, good_c)
    assert rc == _lib.SMH_ERR_INVALID and "row_perm[40] = 4000000000 is not below %d" % n_rows in msg and h is None
    # a repeated value: its second occurrence is the offending position
    bad = good_c.copy()
    bad[[300, 500]] = [7, 7]
    rc, msg, h = _raw_permute(A, good_r, bad)
    assert rc == _lib.SMH_ERR_INVALID and "col_perm[300] = 7 occurs twice" in msg and h is None
    bad = good_c.copy()
    bad[3] = 600  # 600 occurs at 3 and at 600; position 8 is out of range: 8 comes first
    bad[8] = n_cols
    rc, msg, h = _raw_permute(A, None, bad)
    assert rc == _lib.SMH_ERR_INVALID and "col_perm[8] = %d is not below %d" % (n_cols, n_cols) in msg and h is None
    with pytest.raises(sm.SparseMatPanic) as e:
        A.permute(col_perm=bad)
    assert e.value.status == _lib.SMH_ERR_INVALID
    _same(A, (off, col, val), n_rows, n_cols)
    # not square
    with pytest.raises(sm.SparseMatPanic) as e:
        A.permute_symmetric(good_r)
    assert e.value.status == _lib.SMH_ERR_NOT_SQUARE and "Matrix is not symmetric" in str(e.value)
    with pytest.raises(sm.SparseMatPanic) as e:
        A.rcm()
    assert e.value.status == _lib.SMH_ERR_NOT_SQUARE
    _same(A, (off, col, val), n_rows, n_cols)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_vector_gather_and_scatter(gpu, dtype):
    rng = np.random.default_rng(31)
    n = 1003  # not a multiple of 4
    x = rng.standard_normal(n).astype(dtype)
    x[:4] = [np.nan, -0.0, np.inf, -np.inf]
    p = rng.permutation(n).astype(np.uint32)
    X = sm.DenseVec.from_vec(x)
    G = X.permute(p)
    assert (_bits(G.to_numpy()) == _bits(rm.vec_permute(x, p))).all()
    S = X.permute(p, inverse=True)
    assert (_bits(S.to_numpy()) == _bits(rm.vec_permute(x, p, True))).all()
    assert (_bits(G.permute(p, inverse=True).to_numpy()) == _bits(x)).all()
    assert (_bits(X.to_numpy()) == _bits(x)).all()
    for bad, status, text in ((p[:-1], _lib.SMH_ERR_DIM_MISMATCH, "perm has 1002 entries, 1003 expected"),
                              (np.where(np.arange(n) == 77, n, p), _lib.SMH_ERR_INVALID, "perm[77] = 1003 is not below 1003"),
                              (np.where(np.arange(n) == 500, p[2], p), _lib.SMH_ERR_INVALID, "perm[500] = %d occurs twice" % p[2])):
        with pytest.raises(sm.SparseMatPanic) as e:
            X.permute(bad)
        assert e.value.status == status and text in str(e.value)
    Y = sm.DenseVec.zeros(n + 1, dtype)
    assert sm.lib().smh_vec_permute(Y._h, X._h, p.ctypes.data, n, 0) == _lib.SMH_ERR_DIM_MISMATCH
    assert sm.lib().smh_vec_permute(X._h, X._h, p.ctypes.data, n, 0) == _lib.SMH_ERR_INVALID


def _product_inputs(dtype):
    n, off, col, val = rm.grid2d(24, 17, dtype)
    (off, col, val), _ = rm.renumber(n, off, col, val, seed=7)
    yield "grid24x17", n, off, col, val
    rng = np.random.default_rng(37)
    n = 2000
    off, col, val = util.random_crs(rng, n, n, rng.integers(1, 201, n), dtype)
    yield "random2000", n, off, col, val


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_product_identity_through_the_storage_order_kernels(gpu, dtype):
    """B = P A P^T keeps every row's entries in storage order, so SEQ and STREAM give B x[p] == (A x)[p] bit for bit; AUTO is held
    to the parity bound against the oracle on B's arrays."""
    for name, n, off, col, val in _product_inputs(dtype):
        rng = np.random.default_rng(41)
        x = rng.uniform(-1.0, 1.0, n).astype(dtype)
        p = rng.permutation(n).astype(np.uint32)
        A = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
        B = A.permute_symmetric(p)
        for variant in ("seq", "stream"):
            ya, yb = A.mvp(x, variant), B.mvp(x[p], variant)
            assert (_bits(yb) == _bits(ya[p])).all(), (name, variant)
        bo, bc, bv = B.raw_parts()
        util.assert_spmv_close(B.mvp(x[p], "auto"), bo, bc, bv, x[p], what="%s auto" % name)


def test_dev_forms(gpu):
    """the _dev entry points read the permutation from device memory"""
    rng = np.random.default_rng(43)
    n = 700
    off, col, val = util.random_crs(rng, n, n, rng.integers(0, 9, n), np.float32)
    A = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    p = rng.permutation(n).astype(np.uint32)
    P = sm.DenseVec.from_vec(p.view(np.float32))  # n u32 in device memory
    h = C.c_void_p()
    _lib.check(sm.lib().smh_crs_permute_symmetric_dev(A._h, C.c_void_p(P.data_ptr()), n, C.byref(h)))
    _same(sm.SparseMatCRS(h, np.float32), rm.permute_symmetric(n, off, col, val, p), n, n)
    h = C.c_void_p()
    _lib.check(sm.lib().smh_crs_permute_dev(A._h, C.c_void_p(P.data_ptr()), n, None, 0, C.byref(h)))
    _same(sm.SparseMatCRS(h, np.float32), rm.permute(n, n, off, col, val, p, None), n, n)
    x = rng.standard_normal(n).astype(np.float32)
    X, Y = sm.DenseVec.from_vec(x), sm.DenseVec.zeros(n, np.float32)
    _lib.check(sm.lib().smh_vec_permute_dev(Y._h, X._h, C.c_void_p(P.data_ptr()), n, 1))
    assert (Y.to_numpy() == rm.vec_permute(x, p, True)).all()
    out = sm.DenseVec.zeros(n, np.float32)
    comps, levels = C.c_size_t(), C.c_size_t()
    _lib.check(sm.lib().smh_crs_rcm_dev(A._h, C.c_void_p(out.data_ptr()), C.byref(comps), C.byref(levels)))
    want, wc, wl = rm.rcm(n, off, col)
    assert (out.to_numpy().view(np.uint32) == want).all() and (comps.value, levels.value) == (wc, wl)
