"""GPU: every entry point that exists as a host form and a _dev form gives the same answer through both, bit for bit: every
output array, every scalar out-parameter, every smh_last_*_route value.  (Both forms stage their arrays with ArgStage,
csrc/arg_stage.hpp; the helper alone is tests/test_arg_stage_on_host.py.)

Tiny inputs: a 7x6 matrix with row lengths [3, 0, 2, 4, 1, 0, 2], unsorted columns and one repeated (row, column); an 8x8
symmetric pattern of three components (a path of 5 vertices, an isolated vertex, a pair) for the square-only calls; a matrix
with rows and no entries; SparseMatCRS.new(), which has no rows.  Device arrays come from smh_dev_alloc / smh_dev_upload."""
import ctypes as C

import numpy as np
import pytest

import sparsemat_amd as sm
from sparsemat_amd import _lib

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]

R_OFF = np.array([0, 3, 3, 5, 9, 10, 10, 12], np.uint32)
R_COL = np.array([4, 1, 4, 5, 0, 3, 0, 2, 1, 2, 5, 3], np.uint32)  # (0, 4) twice
R_ROWS, R_COLS = 7, 6
# path 3 - 6 - 0 - 5 - 1, isolated 4, pair 2 - 7; some diagonals; columns unsorted
S_ADJ = {0: [6, 0, 5], 1: [5], 2: [7, 2], 3: [6, 3], 4: [], 5: [1, 0], 6: [0, 3, 6], 7: [2]}
S_N = 8


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _values(n, dtype, seed):
    v = np.random.default_rng(seed).standard_normal(n).astype(dtype)
    if n > 3:
        v[1], v[3] = -0.0, np.inf
    return v


def _rect(dtype):
    return sm.SparseMatCRS.from_raw_parts(R_ROWS, R_COLS, R_OFF, R_COL, _values(len(R_COL), dtype, 1))


def _sym(dtype):
    off = np.cumsum([0] + [len(S_ADJ[i]) for i in range(S_N)]).astype(np.uint32)
    col = np.array([j for i in range(S_N) for j in S_ADJ[i]], np.uint32)
    return sm.SparseMatCRS.from_raw_parts(S_N, S_N, off, col, _values(len(col), dtype, 2))


def _no_entries(dtype, n_rows=4, n_cols=4):
    return sm.SparseMatCRS.from_raw_parts(n_rows, n_cols, np.zeros(n_rows + 1, np.uint32), [], np.zeros(0, dtype))


class Dev:
    """a device array: smh_dev_alloc, filled from `host` (smh_dev_upload) or with the byte 0xA5"""

    def __init__(self, host=None, nbytes=0):
        self.host = None if host is None else np.ascontiguousarray(host)
        self.nbytes = nbytes if host is None else self.host.nbytes
        p = C.c_void_p()
        _lib.check(sm.lib().smh_dev_alloc(self.nbytes, C.byref(p)))
        self.ptr = p.value
        if host is None:
            _lib.check(sm.lib().smh_dev_memset(C.c_void_p(self.ptr), 0xA5, self.nbytes, None))
            _lib.check(sm.lib().smh_device_synchronize())
        else:
            _lib.check(sm.lib().smh_dev_upload(C.c_void_p(self.ptr), self.host.ctypes.data, self.nbytes))

    def get(self, dtype):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype)
        _lib.check(sm.lib().smh_dev_download(out.ctypes.data, C.c_void_p(self.ptr), out.nbytes))
        return out

    def __del__(self):
        if getattr(self, "ptr", None):
            sm.lib().smh_dev_free(C.c_void_p(self.ptr))
            self.ptr = None


def _p(a):
    """what the C ABI takes: the data pointer of a numpy array or of a Dev, NULL for None"""
    if a is None:
        return None
    return C.c_void_p(a.ptr) if isinstance(a, Dev) else C.c_void_p(a.ctypes.data)


def _dev(a):
    return None if a is None else Dev(a)


def _state(m):
    o, c, v = m.raw_parts()
    return (m.n_rows(), m.n_cols(), m.n_non_zero_entries(), m.orphans(), o.tobytes(), c.tobytes(), _bits(v).tobytes())


def _filled(n, dtype):
    return np.frombuffer(b"\xa5" * (n * np.dtype(dtype).itemsize), dtype).copy()


# ---- column_info ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [_rect, _no_entries, sm.SparseMatCRS.new], ids=["7x6", "no_entries", "new"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_column_info(gpu, make, dtype):
    A = make(dtype)
    nnz, n_cols = A.n_non_zero_entries(), A.n_cols()
    host = [_filled(max(nnz, 1), np.uint32), _filled(n_cols + 1, np.uint32), _filled(max(nnz, 1), np.uint32)]
    dev = [Dev(nbytes=h.nbytes) for h in host]
    _lib.check(sm.lib().smh_crs_column_info(A._h, *[_p(h) for h in host]))
    _lib.check(sm.lib().smh_crs_column_info_dev(A._h, *[_p(d) for d in dev]))
    for h, d, n in zip(host, dev, (nnz, n_cols + 1, nnz)):
        assert (h[:n] == d.get(np.uint32)[:n]).all()
    if make is _rect:
        assert host[1][-1] == nnz and sorted(host[2]) == list(range(nnz))


# ---- permute, permute_symmetric, vec_permute ----------------------------------------------------------------------------------
def _permute(A, rp, cp, dev):
    fn = sm.lib().smh_crs_permute_dev if dev else sm.lib().smh_crs_permute
    r, c = (_dev(rp), _dev(cp)) if dev else (rp, cp)
    h = C.c_void_p()
    _lib.check(fn(A._h, _p(r), 0 if rp is None else len(rp), _p(c), 0 if cp is None else len(cp), C.byref(h)))
    return _state(sm.SparseMatCRS(h, A.dtype))


@pytest.mark.parametrize("form", ["rows", "cols", "both"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_permute(gpu, dtype, form):
    rp = np.array([5, 0, 6, 2, 1, 4, 3], np.uint32) if form != "cols" else None
    cp = np.array([2, 5, 0, 1, 4, 3], np.uint32) if form != "rows" else None
    A = _rect(dtype)
    want = _permute(A, rp, cp, False)
    assert want == _permute(A, rp, cp, True)
    assert want != _state(A) and want[:4] == _state(A)[:4]
    E = _no_entries(dtype, 7, 6)
    assert _permute(E, rp, cp, False) == _permute(E, rp, cp, True)
    Z = sm.SparseMatCRS.new(dtype)
    assert _permute(Z, None, None, False) == _permute(Z, None, None, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_permute_symmetric(gpu, dtype):
    p = np.array([7, 3, 0, 4, 6, 1, 5, 2], np.uint32)
    A = _sym(dtype)
    out = []
    for fn, arg in ((sm.lib().smh_crs_permute_symmetric, p), (sm.lib().smh_crs_permute_symmetric_dev, Dev(p))):
        h = C.c_void_p()
        _lib.check(fn(A._h, _p(arg), len(p), C.byref(h)))
        out.append(_state(sm.SparseMatCRS(h, dtype)))
    assert out[0] == out[1] and out[0] != _state(A)


@pytest.mark.parametrize("inverse", [0, 1], ids=["forward", "inverse"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vec_permute(gpu, dtype, inverse):
    p = np.array([4, 0, 6, 1, 5, 2, 3], np.uint32)
    x = _values(7, dtype, 3)
    X = sm.DenseVec.from_vec(x)
    out = []
    for fn, arg in ((sm.lib().smh_vec_permute, p), (sm.lib().smh_vec_permute_dev, Dev(p))):
        Y = sm.DenseVec.zeros(7, dtype)
        _lib.check(fn(Y._h, X._h, _p(arg), 7, inverse))
        out.append(_bits(Y.to_numpy()))
    assert (out[0] == out[1]).all()
    want = np.empty_like(x)
    if inverse:
        want[p] = x
    else:
        want = x[p]
    assert (out[0] == _bits(want)).all()


# ---- rcm, color ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [_sym, _no_entries, sm.SparseMatCRS.new], ids=["8x8", "no_entries", "new"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rcm(gpu, make, dtype):
    A = make(dtype)
    n = A.n_rows()
    out = []
    for fn, perm in ((sm.lib().smh_crs_rcm, _filled(max(n, 1), np.uint32)), (sm.lib().smh_crs_rcm_dev, Dev(nbytes=4 * max(n, 1)))):
        comps, levels = C.c_size_t(77), C.c_size_t(77)
        _lib.check(fn(A._h, _p(perm), C.byref(comps), C.byref(levels)))
        got = perm.get(np.uint32) if isinstance(perm, Dev) else perm
        out.append((got[:n].tolist(), comps.value, levels.value))
    assert out[0] == out[1]
    assert sorted(out[0][0]) == list(range(n))
    if make is _sym:
        assert out[0][1] == 3


@pytest.mark.parametrize("which", ["both", "colors", "perm", "neither"])
@pytest.mark.parametrize("make", [_sym, _no_entries, sm.SparseMatCRS.new], ids=["8x8", "no_entries", "new"])
def test_color(gpu, make, which):
    A = make(np.float64)
    n = A.n_rows()
    out = []
    for dev in (False, True):
        fn = sm.lib().smh_crs_color_dev if dev else sm.lib().smh_crs_color
        arrays = [(Dev(nbytes=4 * max(n, 1)) if dev else _filled(max(n, 1), np.uint32)) if which in ("both", name) else None
                  for name in ("colors", "perm")]
        n_colors, n_rounds = C.c_size_t(77), C.c_size_t(77)
        _lib.check(fn(A._h, 9, _p(arrays[0]), _p(arrays[1]), C.byref(n_colors), C.byref(n_rounds)))
        got = [None if a is None else (a.get(np.uint32) if dev else a)[:n].tolist() for a in arrays]
        out.append((got, n_colors.value, n_rounds.value))
    assert out[0] == out[1]
    if make is _sym and which == "both":
        colors, perm = out[0][0]
        assert sorted(perm) == list(range(n)) and max(colors) + 1 == out[0][1]
        assert all(colors[i] != colors[j] for i in range(n) for j in S_ADJ[i] if i != j)


# ---- get_many --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [_rect, _no_entries, sm.SparseMatCRS.new], ids=["7x6", "no_entries", "new"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_get_many(gpu, make, dtype):
    A = make(dtype)
    # present, the repeated pair (the first of the two answers), absent in a row, an empty row, rows >= n_rows, a column no entry has
    rows = np.array([0, 0, 3, 6, 2, 1, 4, 7, 100, 0xFFFFFFFF, 3], np.uint32)
    cols = np.array([4, 1, 2, 3, 1, 0, 2, 0, 4, 0, 0xFFFFFFFF], np.uint32)
    host = _filled(len(rows), dtype)
    dev, d_rows, d_cols = Dev(nbytes=host.nbytes), Dev(rows), Dev(cols)
    _lib.check(sm.lib().smh_crs_get_many(A._h, len(rows), _p(rows), _p(cols), _p(host)))
    _lib.check(sm.lib().smh_crs_get_many_dev(A._h, len(rows), _p(d_rows), _p(d_cols), _p(dev)))
    assert (_bits(host) == _bits(dev.get(dtype))).all()
    if make is _rect:
        v = _values(len(R_COL), dtype, 1)
        assert (_bits(host) == _bits(np.array([v[0], v[1], v[7], v[11], 0, 0, v[9], 0, 0, 0, 0], dtype))).all()
    else:
        assert (_bits(host) == 0).all()


# ---- apply -----------------------------------------------------------------------------------------------------------------------
def _apply_both(make, rows, cols, vals, ops):
    """-> the state and the route after the host form and after the _dev form, each on a matrix of its own"""
    rows, cols = np.asarray(rows, np.uint32), np.asarray(cols, np.uint32)
    ops = None if ops is None else np.asarray(ops, np.uint8)
    out = []
    for dev in (False, True):
        A = make()
        fn = sm.lib().smh_crs_apply_dev if dev else sm.lib().smh_crs_apply
        args = [_dev(a) if dev else a for a in (rows, cols, vals, ops)]
        _lib.check(fn(A._h, len(rows), *[_p(a) for a in args]))
        out.append((_state(A), sm.lib().smh_last_apply_route()))
    return out


@pytest.mark.parametrize("with_ops", [False, True], ids=["add_to", "ops"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_apply(gpu, dtype, with_ops):
    before = _state(_rect(dtype))
    # values only: existing entries, one of them twice, the repeated pair (its first entry takes it)
    rows, cols = [3, 0, 6, 3, 0], [2, 4, 5, 2, 1]
    h, d = _apply_both(lambda: _rect(dtype), rows, cols, _values(5, dtype, 4), [0, 1, 0, 0, 1] if with_ops else None)
    assert h == d and h[1] == 1 and h[0] != before and h[0][:6] == before[:6]
    # structural: new entries in a full row, in an empty row and in rows past the last; a new column
    rows, cols = [3, 1, 9, 1, 0, 8], [5, 2, 7, 2, 4, 0]
    h, d = _apply_both(lambda: _rect(dtype), rows, cols, _values(6, dtype, 5), [1, 0, 0, 1, 0, 1] if with_ops else None)
    assert h == d and h[1] == 0 and h[0][:3] == (10, 8, 16)
    # replay on a handle without rows: SparseMatCRS.new(), and the state one push leaves (no rows, one orphan)
    rows, cols = [2, 2, 0, 5, 2], [1, 1, 3, 0, 4]
    h, d = _apply_both(lambda: sm.SparseMatCRS.new(dtype), rows, cols, _values(5, dtype, 6), [0, 1, 1, 0, 0] if with_ops else None)
    assert h == d and h[1] == 2 and h[0][0] == 6

    def pushed_once():
        return sm.SparseMatCRS.from_triplets([4], [2], np.array([1.5], dtype), [0], into_crs=True)

    assert pushed_once().n_rows() == 0 and pushed_once().orphans() == 1
    h, d = _apply_both(pushed_once, rows, cols, _values(5, dtype, 6), [0, 1, 1, 0, 0] if with_ops else None)
    assert h == d and h[1] == 2 and h[0][0] == 6


# ---- assemble, replay ------------------------------------------------------------------------------------------------------------
STREAMS = {
    "general": ([3, 1, 3, 0, 5, 1, 3, 0, 5, 2], [2, 0, 2, 4, 1, 3, 0, 4, 1, 2], [0, 1, 0, 0, 1, 0, 1, 1, 0, 0]),
    "one_operation": ([4], [2], [0]),
    "twin_first_pair": ([2, 2, 1, 2, 3], [5, 5, 0, 5, 1], [0, 0, 1, 0, 0]),
    "second_row_below_first": ([4, 1, 4, 2], [7, 0, 1, 3], [1, 0, 0, 0]),
    "nothing": ([], [], []),
}


@pytest.mark.parametrize("with_ops", [False, True], ids=["add_to", "ops"])
@pytest.mark.parametrize("stream", list(STREAMS))
@pytest.mark.parametrize("into_crs", [False, True], ids=["assemble", "replay"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_assemble_and_replay(gpu, dtype, into_crs, stream, with_ops):
    rows, cols, ops = [np.asarray(a, t) for a, t in zip(STREAMS[stream], (np.uint32, np.uint32, np.uint8))]
    n = len(rows)
    vals = _values(n, dtype, 7)
    host = (rows, cols, vals, ops if with_ops else None) if n else (None, None, None, None)
    out = []
    for dev in (False, True):
        fn = getattr(sm.lib(), "smh_crs_%s%s" % ("replay" if into_crs else "assemble", "_dev" if dev else ""))
        args = [_dev(a) if dev else a for a in host]
        h = C.c_void_p()
        _lib.check(fn(_lib.dtype_code(np.dtype(dtype)), n, *[_p(a) for a in args], C.byref(h)))
        out.append(_state(sm.SparseMatCRS(h, dtype)))
    assert out[0] == out[1]
    if into_crs and stream == "one_operation":
        assert out[0][:4] == (0, 3, 0, 1)
    if into_crs and stream == "second_row_below_first":
        assert out[0][3] == 1 and out[0][1] == 8
    if stream == "twin_first_pair":
        assert out[0][2] == (3 if not into_crs else 4)


# ---- update plan -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("from_zero", [0, 1])
@pytest.mark.parametrize("with_ops", [False, True], ids=["add_to", "ops"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_update_plan(gpu, dtype, with_ops, from_zero):
    rows = np.array([3, 0, 6, 3, 0, 3, 4], np.uint32)
    cols = np.array([2, 4, 5, 2, 1, 2, 2], np.uint32)
    ops = np.array([0, 1, 0, 0, 1, 1, 0], np.uint8) if with_ops else None
    vals = _values(len(rows), dtype, 8)
    before = _state(_rect(dtype))
    out = []
    for dev in (False, True):
        A = _rect(dtype)
        create = sm.lib().smh_update_plan_create_dev if dev else sm.lib().smh_update_plan_create
        execute = sm.lib().smh_update_plan_execute_dev if dev else sm.lib().smh_update_plan_execute
        args = [_dev(a) if dev else a for a in (rows, cols, ops)]
        v = _dev(vals) if dev else vals
        h = C.c_void_p()
        _lib.check(create(A._h, len(rows), *[_p(a) for a in args], C.byref(h)))
        plan = sm.sparsemat_crs.UpdatePlan(h, A, len(rows))
        stats = plan.stats()
        _lib.check(execute(plan._h, A._h, _p(v), from_zero))
        once = _state(A)
        _lib.check(execute(plan._h, A._h, _p(v), from_zero))  # (the host form's staging buffer is reused)
        out.append((stats, once, _state(A)))
    assert out[0] == out[1]
    assert out[0][1] != before and out[0][1][:6] == before[:6]
    # an empty plan: create and execute do nothing in both forms
    for dev in (False, True):
        A = _rect(dtype)
        h = C.c_void_p()
        _lib.check((sm.lib().smh_update_plan_create_dev if dev else sm.lib().smh_update_plan_create)(A._h, 0, None, None, None, C.byref(h)))
        plan = sm.sparsemat_crs.UpdatePlan(h, A, 0)
        _lib.check((sm.lib().smh_update_plan_execute_dev if dev else sm.lib().smh_update_plan_execute)(plan._h, A._h, None, from_zero))
        assert _state(A) == before
