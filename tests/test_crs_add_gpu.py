"""SparseMatrix::add / sub (sparsematrix.rs:123-143) and Clone of SparseMatCRS on the device (csrc/matadd.hip): the result of
`a + b`, `a - b`, `a += b`, `a -= b` equals tests/add_model.py (pinned to the literal reference by test_add_model.py) bit for
bit -- offsets, columns, value bits, n_rows, n_cols, orphans -- on every route, the general one forced included; handles stay
usable afterwards (every derived form rebuilt) and borrowed arrays follow the header's two rules."""
import json
import os

import numpy as np
import pytest

import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib, synth
from sparsemat_amd.synth import DeviceBuffer

import add_model
from util import assert_spmv_close

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")
OPS = ("add", "sub", "add_assign", "sub_assign")


def dev(m):
    """(n_rows, n_cols, off, col, val[, orphans]) -> SparseMatCRS (no orphan)"""
    n_rows, n_cols, off, col, val = m[:5]
    return sm.SparseMatCRS.from_raw_parts(n_rows, n_cols, off, col, val, validate=False)


def model_of(h):
    off, col, val = h.raw_parts()
    return (h.n_rows(), h.n_cols(), off, col, val, h.orphans())


def assert_same(h, want, what=""):
    n_rows, n_cols, off, col, val, orph = want
    assert (h.n_rows(), h.n_cols(), h.orphans()) == (n_rows, n_cols, orph), what
    g_off, g_col, g_val = h.raw_parts()
    assert np.array_equal(g_off, np.asarray(off, np.uint32)[:n_rows + 1] if n_rows else np.zeros(1, np.uint32)), what
    assert np.array_equal(g_col, col), what
    assert g_val.dtype == val.dtype and g_val.tobytes() == val.tobytes(), what


def run(make_a, b, op):
    """op on a fresh a (make_a() -> handle); returns the result handle (a itself for the in-place forms)."""
    a = make_a()
    if op == "add":
        return a + b
    if op == "sub":
        return a - b
    if op == "add_assign":
        a += b
        return a
    a -= b
    return a


def check_all(make_a, a_model, b, b_model, what, route=None, forced="general"):
    for general in (False, True):
        os.environ["SMH_ADD_FAST"] = "0" if general else "1"
        try:
            for op in OPS:
                want = add_model.add(a_model, b_model, subtract=op.startswith("sub"))
                h = run(make_a, b, op)
                assert_same(h, want, "%s %s general=%s" % (what, op, general))
                if general:
                    assert sm.SparseMatCRS.last_add_route() == forced, (what, op)
                elif route is not None:
                    assert sm.SparseMatCRS.last_add_route() == route, (what, op)
        finally:
            os.environ.pop("SMH_ADD_FAST", None)


def rand(rng, n_rows, n_cols, max_len, dtype, dup=False):
    lens = rng.integers(0, max_len + 1, n_rows)
    off = np.zeros(n_rows + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    col = rng.integers(0, n_cols, int(off[-1])).astype(np.uint32)
    if dup and len(col) > 1:
        col[1::3] = col[0:-1:3][:len(col[1::3])]
    val = rng.choice(np.array([0.0, -0.0, 1.0, -1.0, 0.5, 3.25], dtype), len(col))
    val = np.where(rng.random(len(col)) < 0.5, val, rng.uniform(-2, 2, len(col))).astype(dtype)
    return (n_rows, n_cols, off, col, val, 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_add_cases_bit_exact(gpu, dtype):
    rng = np.random.default_rng(7 + (dtype == np.float64))
    a = rand(rng, 300, 200, 9, dtype, dup=True)
    a_nodup = rand(rng, 300, 200, 9, dtype)
    for i in range(a_nodup[0]):  # no column repeated inside a row: the same-pattern route applies
        s, e = a_nodup[2][i], a_nodup[2][i + 1]
        a_nodup[3][s:e] = rng.permutation(200)[:e - s]
    diag = (300, 300, np.arange(301, dtype=np.uint32), np.arange(300, dtype=np.uint32), rng.uniform(-1, 1, 300).astype(dtype), 0)
    a_diag = rand(rng, 300, 300, 6, dtype)
    a_diag = (300, 300, *[x for x in _with_diagonal(a_diag, dtype)], 0)
    cases = [
        ("same pattern", a_nodup, (a_nodup[0], a_nodup[1], a_nodup[2], a_nodup[3], (a_nodup[4] * dtype(0.75)).astype(dtype), 0), "same_pattern"),
        ("same pattern with repeats in a", a, (a[0], a[1], a[2], a[3], a[4][::-1].copy(), 0), "structure_unchanged"),
        ("cancellation", a_nodup, a_nodup, "same_pattern"),
        ("subset (diagonal)", a_diag, diag, "structure_unchanged"),
        ("disjoint", a_nodup, (300, 400, a_nodup[2], (a_nodup[3] + 200).astype(np.uint32), a_nodup[4], 0), "short_rows"),
        ("duplicates on both sides", a, rand(rng, 300, 200, 9, dtype, dup=True), "short_rows"),
        ("b grows rows and columns", a, rand(rng, 450, 260, 5, dtype, dup=True), "short_rows"),
        ("b smaller, trailing empty rows", a, (5, 3, np.array([0, 2, 2, 3, 3, 3], np.uint32), np.array([1, 250, 1], np.uint32),
                                               np.array([1.5, -2.0, 0.25], dtype), 0), "short_rows"),
        ("empty b", a, (4, 9, np.zeros(5, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype), 0), "structure_unchanged"),
    ]
    for what, am, bm, route in cases:
        b = dev(bm)
        check_all(lambda: dev(am), am, b, bm, what, route, "structure_unchanged" if what == "empty b" else "general")


def _with_diagonal(m, dtype):
    """m's rows with the diagonal appended where missing -> (off, col, val)"""
    n_rows, _, off, col, val, _ = m
    offs, cols, vals = [0], [], []
    for i in range(n_rows):
        c, v = list(col[off[i]:off[i + 1]]), list(val[off[i]:off[i + 1]])
        if i not in c:
            c.append(i)
            v.append(dtype(4.0))
        cols += c
        vals += v
        offs.append(len(cols))
    return np.array(offs, np.uint32), np.array(cols, np.uint32), np.array(vals, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_add_without_rows_and_orphans(gpu, dtype):
    rng = np.random.default_rng(11)
    b_m = rand(rng, 40, 30, 4, dtype, dup=True)
    b = dev(b_m)
    # a without rows and without an orphan: the replay of b's stream (as smh_crs_replay), n_cols at least a's
    for n_cols in (0, 100):
        empty = (0, n_cols, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype), 0)
        check_all(lambda: dev(empty), empty, b, b_m, "a without rows, n_cols %d" % n_cols)
    rows = np.repeat(np.arange(40, dtype=np.uint32), np.diff(b_m[2].astype(np.int64)))
    replay = sm.SparseMatCRS.from_triplets(rows, b_m[3], b_m[4], into_crs=True)
    s = dev((0, 0, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype))) + b
    assert_same(s, model_of(replay), "== smh_crs_replay")
    # the quirk's orphan and its twin entry through a without rows
    for b2 in ((2, 4, np.array([0, 0, 1], np.uint32), np.array([2], np.uint32), np.array([1.0], dtype), 0),
               (1, 4, np.array([0, 2], np.uint32), np.array([3, 3], np.uint32), np.array([1.0, 2.0], dtype), 0)):
        e = (0, 0, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype), 0)
        check_all(lambda: dev(e), e, dev(b2), b2, "quirk")
    # a with rows and an orphan (second op's row below the first one's): the orphan stays
    def make_orphaned():
        return sm.SparseMatCRS.from_triplets([9, 2, 5, 2, 7], [4, 1, 3, 6, 1], np.array([1, 2, 3, 4, 5], dtype), into_crs=True)
    o = make_orphaned()
    assert o.orphans() == 1 and o.n_rows() > 0
    check_all(make_orphaned, model_of(o), b, b_m, "a with an orphan")


def test_add_errors_leave_a_unchanged(gpu):
    b = dev(rand(np.random.default_rng(3), 10, 10, 3, np.float32))
    lone = sm.SparseMatCRS.from_triplets([3], [2], np.array([1.0], np.float32), into_crs=True)
    assert (lone.n_rows(), lone.orphans()) == (0, 1)
    for fn in (lambda: lone.add(b), lambda: lone.sub(b), lambda: lone + b):
        with pytest.raises(_lib.SparseMatPanic) as e:
            fn()
        assert e.value.status == _lib.SMH_ERR_INVALID and "orphan" in str(e.value)
        assert (lone.n_rows(), lone.n_cols(), lone.orphans()) == (0, 3, 1)
    a = dev(rand(np.random.default_rng(4), 10, 10, 3, np.float64))
    before = model_of(a)
    for fn in (lambda: a.add(b), lambda: a - b):
        with pytest.raises(_lib.SparseMatPanic) as e:
            fn()
        assert e.value.status == _lib.SMH_ERR_INVALID
    assert_same(a, before, "dtype mismatch")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_add_aliasing(gpu, dtype):
    rng = np.random.default_rng(5)
    for m in (rand(rng, 200, 50, 8, dtype), rand(rng, 200, 50, 8, dtype, dup=True)):
        for general in ("1", "0"):
            os.environ["SMH_ADD_FAST"] = general
            try:
                for sub in (False, True):
                    a = dev(m)
                    if sub:
                        a -= a
                    else:
                        a += a
                    assert_same(a, add_model.add(m, m, sub), "a op= a")
                    a = dev(m)
                    assert_same(a + a, add_model.add(m, m), "a + a")
            finally:
                os.environ.pop("SMH_ADD_FAST", None)


def test_add_long_rows(gpu):
    rng = np.random.default_rng(9)
    lens = np.array([70_000, 3_000, 5, 0, 2_100], np.int64)
    def mk(n_cols, dup):
        off = np.zeros(len(lens) + 1, np.uint32)
        off[1:] = np.cumsum(lens)
        col = rng.integers(0, n_cols, int(off[-1])).astype(np.uint32)
        if dup:
            col[1::5] = col[0:-1:5][:len(col[1::5])]
        return (len(lens), n_cols, off, col, rng.uniform(-1, 1, len(col)).astype(np.float32), 0)
    a_m, b_m = mk(90_000, True), mk(120_000, True)
    check_all(lambda: dev(a_m), a_m, dev(b_m), b_m, "long rows", "general")
    check_all(lambda: dev(a_m), a_m, dev(a_m), a_m, "long rows, same pattern", "general")


def test_add_laplacian_shift_and_powerlaw(gpu):
    g = 128
    off, col, val = oracle.laplace3d(g, g, g, np.float32)
    n = g ** 3
    lap = (n, n, off, col, val, 0)
    shift = (n, n, np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.full(n, 0.125, np.float32), 0)
    a = dev(lap)
    s = dev(shift)
    r = a + s
    assert sm.SparseMatCRS.last_add_route() == "structure_unchanged"
    assert_same(r, add_model.add(lap, shift), "A + sigma I")
    a -= a
    assert sm.SparseMatCRS.last_add_route() == "same_pattern"
    assert_same(a, add_model.add(lap, lap, True), "A -= A")
    # power law (a few million rows) plus its transpose: long rows, the general route
    p = synth.crs_powerlaw(0x5EED0003, 2_000_000, 2_000_000, np.float64, kmax=3000, alpha=2.2)
    pt = p.transpose()
    pm, ptm = model_of(p), model_of(pt)
    s = p + pt
    assert sm.SparseMatCRS.last_add_route() == "general"
    assert_same(s, add_model.add(pm, ptm), "P + P^T")


def _kat_sp():
    case = json.load(open(GOLDEN))["cases"][0]
    rows = [o[1] for o in case["ops"]]
    return sm.SparseMatCRS.from_triplets(rows, [o[2] for o in case["ops"]], np.array([np.float32(o[3]) for o in case["ops"]]),
                                         [1 if o[0] == "set" else 0 for o in case["ops"]])


def _get(h, i, j):
    for c, v in h.iter_row(i):
        if c == j:
            return v
    return h.dtype.type(0)


def test_reference_known_answers_on_device(gpu):
    sp = _kat_sp()
    ssum = sp.clone() + sp.clone()
    assert _get(ssum, 0, 0) == np.float32(14.24)                       # lib.rs:74-75
    diff = ssum.clone() - sp.clone()
    assert _get(diff, 0, 0) == _get(sp, 0, 0)                          # :76-77
    mul = sp.clone() * 2.0
    assert _get(mul, 0, 0) == _get(ssum, 0, 0)                         # :78-79
    sp2 = sp.clone()
    sp2 += sp
    assert [float(_get(sp2, 1, j)) for j in range(3)] == [0.0, float(np.float32(4.48)), float(np.float32(8.24))]  # :104-107
    # Mul<T> on a clone leaves the original alone; A * DenseVec / array is the product as before
    x = np.array([2.0, 4.8, 1.2], np.float32)
    assert sp.mvp(x).tobytes() == (sp * x).tobytes()
    assert (sp * x)[0] == np.float32(34.544)
    m2 = sp.clone()
    m2 *= 2.0
    assert model_of(m2)[4].tobytes() == model_of(mul)[4].tobytes()


def test_clone_is_independent(gpu):
    a = dev(rand(np.random.default_rng(12), 50, 40, 6, np.float64))
    a.set_vector_lanes(4)
    before = model_of(a)
    c = a.clone()
    assert_same(c, model_of(a), "clone")
    assert c.resolved_variant() == a.resolved_variant()
    c.scale(3.0)
    bm = rand(np.random.default_rng(13), 60, 70, 3, np.float64)
    want = add_model.add(model_of(c), bm)
    c += dev(bm)
    assert_same(c, want, "clone += b")
    assert_same(a, before, "original untouched")


def test_handle_usable_after_add_assign(gpu):
    """Every derived form of a built first (K1s with the XD-V dictionary, K1 / K1r, merge tiles, K2t, K2c), then a += b with
    new values and new entries: SEQ and STREAM equal the oracle's product of the model bit for bit, the others pass the gate."""
    g = 300
    off, col, val = oracle.laplace2d(g, g, np.float32)
    n = g * g
    a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    x = oracle.gen_x(synth.SEED_X, n, np.float32)
    a.set_stream_xs(1)
    a.set_colblock_shift(12)
    a.mvp(x, variant="stream")
    assert a.stream_direct() and len(a.stream_value_dict()) == 2  # the dictionary is active
    for v in ("vector", "merge", "tiled", "colblock"):
        a.mvp(x, variant=v)
    b_rows = np.repeat(np.arange(n, dtype=np.int64), 2)
    b_off = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
    b_col = np.empty(2 * n, np.uint32)
    b_col[0::2] = col[off[:-1]]                                 # lands on an existing entry
    b_col[1::2] = (b_rows[1::2] * 7 + 3) % n                    # mostly new entries
    b_val = np.where(np.arange(2 * n) % 2 == 0, 0.375, -3.5).astype(np.float32)  # values the dictionary does not hold
    bm = (n, n, b_off, b_col, b_val, 0)
    want = add_model.add((n, n, off, col, val, 0), bm)
    a += dev(bm)
    assert_same(a, want, "a += b")
    w_off, w_col, w_val = want[2], want[3], want[4]
    y_ref = oracle.spmv(w_off, w_col, w_val, x)
    for v in ("seq", "stream"):
        assert a.mvp(x, variant=v).tobytes() == y_ref.tobytes(), v
    for v in ("vector", "merge", "tiled", "colblock", "auto"):
        assert_spmv_close(a.mvp(x, variant=v), w_off, w_col, w_val, x, v)


def test_borrowed_arrays(gpu):
    rng = np.random.default_rng(31)
    m = rand(rng, 500, 300, 7, np.float32)
    n_rows, n_cols, off, col, val, _ = m
    bufs = [DeviceBuffer(max(len(a), 4) * 4 + 16) for a in (off, col, val)]
    for buf, arr in zip(bufs, (off, col, val)):
        buf.upload(arr)
    def borrowed():
        return sm.SparseMatCRS.from_device_parts(n_rows, n_cols, len(val), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, np.float32, keep=bufs)
    # structure unchanged: the lent values are updated in place
    a = borrowed()
    b_same = dev((n_rows, n_cols, off, col, np.full(len(val), 0.5, np.float32)))
    want = add_model.add(m, (n_rows, n_cols, off, col, np.full(len(val), 0.5, np.float32), 0))
    a += b_same
    assert_same(a, want, "borrowed, same structure")
    assert bufs[2].download(np.float32, len(val)).tobytes() == want[4].tobytes()
    assert np.array_equal(bufs[1].download(np.uint32, len(col)), col)
    # structure grows: the handle moves to its own arrays, the lent ones are not written
    before = [buf.download(np.uint8, buf.nbytes) for buf in bufs]
    a = borrowed()
    cur = model_of(a)
    bm = rand(rng, 520, 320, 3, np.float32)
    a += dev(bm)
    assert_same(a, add_model.add(cur, bm), "borrowed, grows")
    after = [buf.download(np.uint8, buf.nbytes) for buf in bufs]
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
