"""SparseMatrix::get / set / add_to / eye of SparseMatCRS on the device (csrc/matupdate.hip): `apply` of a set / add_to stream
equals tests/update_model.py (pinned to the literal reference by test_update_model.py) bit for bit -- offsets, columns, value
bits, n_rows, n_cols, orphans -- on every route, the general one forced included, host and device forms; it agrees with
`a += b` and with assembly of the joined stream; products stay right after a values-only update; borrowed arrays, errors,
the recorded first push and batched lookups behave as the header says."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib, synth
from sparsemat_amd._lib import lib
from sparsemat_amd.synth import DeviceBuffer

import update_model
from oracle.assembly import CrsPushMatrix
from test_crs_add_gpu import assert_same, dev, model_of, rand
from test_update_model import random_stream, run_stream, state

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")


def upload(arr):
    a = np.ascontiguousarray(arr)
    buf = DeviceBuffer(a.nbytes + 16)
    if a.nbytes:
        buf.upload(a)
    return buf


def apply_on(h, rows, cols, vals, ops, form):
    vals = np.asarray(vals, h.dtype)
    if form == "host":
        h.apply(rows, cols, vals, ops)
        return
    bufs = [upload(np.asarray(rows, np.uint32)), upload(np.asarray(cols, np.uint32)), upload(vals)]
    ob = None if ops is None else upload(np.asarray(ops, np.uint8))
    h.apply_dev(len(vals), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None if ob is None else ob.ptr)


def check_apply(make_m, m_model, rows, cols, vals, ops, what, route=None, first=None, forms=("host", "dev")):
    want = update_model.apply(m_model, rows, cols, vals, ops, first=first)
    for general in (False, True):
        os.environ["SMH_APPLY_FAST"] = "0" if general else "1"
        try:
            for form in forms:
                h = make_m()
                apply_on(h, rows, cols, vals, ops, form)
                assert_same(h, want, "%s general=%s %s" % (what, general, form))
                got = sm.SparseMatCRS.last_apply_route()
                if m_model[0] == 0:
                    assert got == "replay", what
                elif general and len(vals):
                    assert got == "general", what
                elif route is not None:
                    assert got == route, what
        finally:
            os.environ.pop("SMH_APPLY_FAST", None)
    return want


def existing_pairs(m, rng, n):
    n_rows, _, off, col = m[:4]
    rows_m = np.repeat(np.arange(n_rows, dtype=np.uint32), np.diff(off.astype(np.int64)))
    k = rng.integers(0, len(col), n)
    return rows_m[k], col[k].copy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_apply_cases_bit_exact(gpu, dtype):
    rng = np.random.default_rng(101 + (dtype == np.float64))
    a = rand(rng, 300, 200, 9, dtype, dup=True)
    n = 5000
    r_in, c_in = existing_pairs(a, rng, n)
    vals = rng.uniform(-2, 2, n).astype(dtype)
    vals[::7] = dtype(-0.0)
    vals[::11] = np.nan
    ops = (rng.random(n) < 0.3).astype(np.uint8)
    check_apply(lambda: dev(a), a, r_in, c_in, vals, ops, "values only", "values_only")
    check_apply(lambda: dev(a), a, r_in, c_in, vals, None, "values only, ops=None", "values_only")
    r_new = rng.integers(0, 400, n).astype(np.uint32)  # rows beyond n_rows too
    c_new = rng.integers(0, 260, n).astype(np.uint32)
    check_apply(lambda: dev(a), a, r_new, c_new, vals, ops, "general", "general")
    mix = rng.random(n) < 0.5
    check_apply(lambda: dev(a), a, np.where(mix, r_in, r_new), np.where(mix, c_in, c_new), vals, ops, "mixed", "general")
    check_apply(lambda: dev(a), a, [350], [5], vals[:1], None, "one new entry in a new row", "general")
    check_apply(lambda: dev(a), a, [], [], np.zeros(0, dtype), None, "empty stream", "values_only")
    # small random cases of the CPU model test, m with rows (an orphan from the replay quirk included)
    for case in range(60):
        if case % 4 == 0:
            h0 = sm.SparseMatCRS.from_triplets([3, 1, 2], [1, 0, 2], np.array([1.5, 2.0, -1.0], dtype), into_crs=True)
            m = model_of(h0)
            assert m[5] == 1
            make = lambda: sm.SparseMatCRS.from_triplets([3, 1, 2], [1, 0, 2], np.array([1.5, 2.0, -1.0], dtype), into_crs=True)
        else:
            m = rand(rng, int(rng.integers(1, 8)), int(rng.integers(1, 8)), 5, dtype, dup=True)
            make = lambda m=m: dev(m)
        rows, cols, vals_s, ops_s = random_stream(rng, dtype, m)
        check_apply(make, m, rows, cols, vals_s, ops_s, "random case %d" % case, forms=("host",) if case % 2 else ("dev",))


def test_apply_long_rows(gpu):
    rng = np.random.default_rng(5)
    for max_len in (300, 5000):  # lane groups of 8, of 32
        lens = rng.integers(0, max_len + 1, 400)
        lens[0] = max_len
        off = np.zeros(len(lens) + 1, np.uint32)
        off[1:] = np.cumsum(lens)
        col = rng.integers(0, 20000, int(off[-1])).astype(np.uint32)
        col[1::5] = col[0:-1:5][:len(col[1::5])]
        m = (len(lens), 20000, off, col, rng.uniform(-1, 1, len(col)).astype(np.float32), 0)
        r_in, c_in = existing_pairs(m, rng, 100_000)
        vals = rng.uniform(-1, 1, len(r_in)).astype(np.float32)
        ops = (rng.random(len(vals)) < 0.2).astype(np.uint8)
        check_apply(lambda: dev(m), m, r_in, c_in, vals, ops, "long rows %d, values only" % max_len, "values_only")
        r2 = np.where(rng.random(len(r_in)) < 0.9, r_in, rng.integers(0, 450, len(r_in))).astype(np.uint32)
        c2 = np.where(rng.random(len(r_in)) < 0.9, c_in, rng.integers(0, 30000, len(r_in))).astype(np.uint32)
        check_apply(lambda: dev(m), m, r2, c2, vals, ops, "long rows %d, general" % max_len, "general")
        q = model_of(dev(m))
        assert dev(m).get_many(r2, c2).tobytes() == update_model.get_many(q, r2, c2).tobytes()


def test_without_rows_and_recorded_first_push(gpu):
    rng = np.random.default_rng(9)
    for dtype in (np.float32, np.float64):
        for case in range(30):
            first_rc = (int(rng.integers(0, 5)), int(rng.integers(0, 5)))
            v0, op0 = dtype(rng.choice([1.5, -0.0, 2.25])), int(rng.integers(0, 2))
            rows, cols, vals, ops = random_stream(rng, dtype, (0, 0), nan=False)
            # SparseMatCRS::new()
            want = update_model.apply((0, 0, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype), 0), rows, cols, vals, ops)
            h = sm.SparseMatCRS.new(dtype)
            h.apply(rows, cols, vals, ops)
            assert_same(h, want, "new() case %d" % case)
            assert sm.SparseMatCRS.last_apply_route() == "replay"
            # the one-operation replay keeps its operation: continued as the reference continues it
            c = run_stream(CrsPushMatrix(dtype), [first_rc[0]], [first_rc[1]], [v0], [op0])
            want = state(run_stream(c, rows, cols, vals, ops))
            h = sm.SparseMatCRS.from_triplets([first_rc[0]], [first_rc[1]], np.array([v0], dtype), [op0], into_crs=True)
            assert (h.n_rows(), h.orphans()) == (0, 1)
            h2 = h.clone()
            h.apply(rows, cols, vals, ops)
            assert_same(h, want, "recorded case %d" % case)
            h2.apply(rows, cols, vals, ops)
            assert_same(h2, want, "clone of the recorded state, case %d" % case)


def test_transpose_of_one_entry_continued(gpu):
    a = sm.SparseMatCRS.from_raw_parts(2, 5, np.array([0, 0, 1], np.uint32), np.array([3], np.uint32), np.array([2.5], np.float32))
    t = a.transpose()
    assert (t.n_rows(), t.orphans()) == (0, 1)
    rows, cols, vals, ops = [1, 3, 0, 3], [1, 1, 2, 1], np.array([1.0, 4.0, -2.0, 0.5], np.float32), [0, 0, 1, 0]
    c = run_stream(CrsPushMatrix(np.float32), [3], [1], [np.float32(2.5)], [1])
    t.apply(rows, cols, vals, ops)
    assert_same(t, state(run_stream(c, rows, cols, vals, ops)), "transpose of one entry, continued")


def test_scaled_first_push_continued(gpu):
    """scale multiplies every stored value, the orphaned first push included (sparsemat_crs.rs:153-157); apply brings it back."""
    for dtype in (np.float32, np.float64):
        for make, first in ((lambda: sm.SparseMatCRS.eye(1, dtype), (0, 0, 1.0, 1)),
                            (lambda: sm.SparseMatCRS.from_triplets([2], [1], np.array([0.3], dtype), [0], into_crs=True), (2, 1, 0.3, 0))):
            for how in ("mul", "imul"):
                h = make()
                if how == "mul":
                    h = h * 2.5
                else:
                    h *= 2.5
                rows, cols, vals = [0, 2, 1], [0, 1, 1], np.array([1.0, 0.25, 1.0], dtype)
                c = run_stream(CrsPushMatrix(dtype), [first[0]], [first[1]], [dtype(first[2])], [first[3]])
                c.values = [dtype(v * dtype(2.5)) for v in c.values]
                want = state(run_stream(c, rows, cols, vals, None))
                h.apply(rows, cols, vals)
                assert_same(h, want, "scaled first push (%s), continued" % how)


def test_eye(gpu):
    for dtype in (np.float32, np.float64):
        for dim in range(6):
            h = sm.SparseMatCRS.eye(dim, dtype)
            assert_same(h, update_model.eye(dim, dtype), "eye(%d)" % dim)
        e1 = sm.SparseMatCRS.eye(1, dtype)
        e1.add_to(1, 1, 1.0)
        c = run_stream(CrsPushMatrix(dtype), [0, 1], [0, 1], [dtype(1), dtype(1)], [1, 0])
        assert_same(e1, state(c), "eye(1) continued")
        big = sm.SparseMatCRS.eye(100_000, dtype)
        x = np.random.default_rng(1).uniform(-1, 1, 100_000).astype(dtype)
        assert big.mvp(x).tobytes() == x.tobytes()


def test_reference_crs_test_op_by_op(gpu):
    """src/lib.rs:114-154: the five add_to calls on SparseMatCRS::with_capacity(3), one device call each."""
    case = json.load(open(GOLDEN))["cases"][1]
    assert case["name"] == "check_sparsemat_crs"
    m = sm.SparseMatCRS.new(np.float32)
    for op, i, j, v in case["ops"]:
        assert op == "add_to"
        m.add_to(i, j, np.float32(v))
    crs = case["crs"]
    off, col, val = m.raw_parts()
    assert (m.n_rows(), m.n_cols(), m.orphans()) == (crs["n_rows"], crs["n_cols"], 0)
    assert off.tolist() == crs["offset_rows"] and col.tolist() == crs["columns"]
    assert [hex(b) for b in val.view(np.uint32)] == crs["values_bits"]
    rows_of = np.repeat(np.arange(m.n_rows()), np.diff(off.astype(np.int64)))
    assert [(int(r), int(c), float(v)) for r, c, v in zip(rows_of, col, val)] == \
        [(r, c, float(np.float32(v))) for r, c, v in case["iter_full"]]
    x = np.array([np.float32(s) for s in case["x"]], np.float32)
    assert m.mvp(x)[0] == np.float32(case["expect_mvp"][0][1])
    assert m.density() == 5.0 / 16.0
    assert m.sparsity() == 1.0 - 5.0 / 16.0
    assert m.get(3, 2) == np.float32(1.12) and m.get(0, 0) == 0 and m.get(5, 2) == 0


def test_apply_equals_add_assign(gpu):
    """apply of b's entries in storage order (all add_to) == a += b, on every add route."""
    rng = np.random.default_rng(17)
    a = rand(rng, 300, 200, 9, np.float32, dup=True)
    a_nodup = rand(rng, 300, 200, 9, np.float32)
    for i in range(a_nodup[0]):
        s, e = a_nodup[2][i], a_nodup[2][i + 1]
        a_nodup[3][s:e] = rng.permutation(200)[:e - s]
    pairs = [(a_nodup, (300, 200, a_nodup[2], a_nodup[3], (a_nodup[4] * 0.75).astype(np.float32), 0)),
             (a, (300, 200, a[2], a[3], a[4][::-1].copy(), 0)),
             (a, rand(rng, 450, 260, 5, np.float32, dup=True))]
    for fast in ("1", "0"):
        os.environ["SMH_ADD_FAST"] = fast
        try:
            for am, bm in pairs:
                x = dev(am)
                x += dev(bm)
                route = sm.SparseMatCRS.last_add_route()
                y = dev(am)
                rows_b = np.repeat(np.arange(bm[0], dtype=np.uint32), np.diff(bm[2].astype(np.int64)))
                y.apply(rows_b, bm[3], bm[4])
                assert_same(y, model_of(x), "apply vs += (%s)" % route)
        finally:
            os.environ.pop("SMH_ADD_FAST", None)


def hex_stream(g, dtype, rng):
    nodes = np.arange((g + 1) ** 3, dtype=np.uint32).reshape(g + 1, g + 1, g + 1)
    corners = np.stack([nodes[dx:g + dx, dy:g + dy, dz:g + dz].ravel()
                        for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)], axis=1)
    rows = np.repeat(corners, 8, axis=1).ravel()
    cols = np.tile(corners, (1, 8)).ravel()
    vals = rng.uniform(-1, 1, len(rows)).astype(dtype)
    return rows, cols, vals


def test_reassembly_equals_assembly_of_joined_stream(gpu):
    rng = np.random.default_rng(3)
    r1, c1, v1 = hex_stream(64, np.float32, rng)
    r2, c2, v2 = hex_stream(64, np.float32, rng)
    perm = rng.permutation(len(r2))[: len(r2) // 2]
    r2, c2, v2 = r2[perm], c2[perm], v2[perm]
    ops2 = (rng.random(len(v2)) < 0.1).astype(np.uint8)
    ops = np.r_[np.zeros(len(v1), np.uint8), ops2]
    joined = sm.SparseMatCRS.from_triplets(np.r_[r1, r2], np.r_[c1, c2], np.r_[v1, v2], ops)
    want = model_of(joined)
    for fast in ("1", "0"):
        os.environ["SMH_APPLY_FAST"] = fast
        try:
            m = sm.SparseMatCRS.from_triplets(r1, c1, v1)
            m.apply(r2, c2, v2, ops2)
            assert sm.SparseMatCRS.last_apply_route() == ("values_only" if fast == "1" else "general")
            assert_same(m, want, "assemble(S1).apply(S2), fast=%s" % fast)
        finally:
            os.environ.pop("SMH_APPLY_FAST", None)


VARIANTS = ("vector", "merge", "seq", "stream", "colblock", "colfused", "colsplit", "tiled", "auto")


def _configured(n, off, col, val):
    h = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    h.set_stream_xs(1)
    h.set_colblock_shift(12)
    return h


@pytest.mark.parametrize("dict_before", [True, False])
def test_products_after_values_only_apply(gpu, dict_before):
    g = 300
    off, col, val = oracle.laplace2d(g, g, np.float32)
    n = g * g
    rng = np.random.default_rng(23)
    if not dict_before:
        val = rng.uniform(-1, 1, len(val)).astype(np.float32)  # > 32 distinct values: no dictionary
    a = _configured(n, off, col, val)
    x = oracle.gen_x(synth.SEED_X, n, np.float32)
    ran = []
    for v in VARIANTS:  # every derived form built before the update
        try:
            a.prepare(v)
        except _lib.SparseMatPanic:
            continue
        a.mvp(x, variant=v)
        ran.append(v)
    assert {"vector", "merge", "seq", "stream", "colblock", "tiled"} <= set(ran)
    assert (len(a.stream_value_dict()) > 0) == dict_before
    rows_m = np.repeat(np.arange(n, dtype=np.uint32), np.diff(off.astype(np.int64)))
    if dict_before:  # new values everywhere: the dictionary stops applying
        k = rng.permutation(len(col))
        a.apply(rows_m[k], col[k], rng.uniform(-1, 1, len(k)).astype(np.float32))
    else:  # every entry set to one of two values: the dictionary applies afterwards
        a.apply(rows_m, col, np.where(col == rows_m, 4.0, -1.0).astype(np.float32), np.ones(len(col), np.uint8))
    assert sm.SparseMatCRS.last_apply_route() == "values_only"
    g_off, g_col, g_val = a.raw_parts()
    fresh = _configured(n, g_off, g_col, g_val)
    for v in ran:
        assert a.mvp(x, variant=v).tobytes() == fresh.mvp(x, variant=v).tobytes(), v
    assert (len(a.stream_value_dict()) > 0) == (not dict_before)
    assert a.stream_value_dict().tobytes() == fresh.stream_value_dict().tobytes()


def test_borrowed_arrays(gpu):
    rng = np.random.default_rng(31)
    m = rand(rng, 500, 300, 7, np.float32, dup=True)
    n_rows, n_cols, off, col, val, _ = m
    bufs = [upload(a) for a in (off, col, val)]

    def borrowed():
        return sm.SparseMatCRS.from_device_parts(n_rows, n_cols, len(val), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, np.float32, keep=bufs)

    a = borrowed()
    cur = m
    for step in range(2):  # values only, twice: written into the lent array, still borrowing
        r, c = existing_pairs(m, rng, 3000)
        v = rng.uniform(-1, 1, 3000).astype(np.float32)
        cur = update_model.apply(cur, r, c, v)
        a.apply(r, c, v)
        assert sm.SparseMatCRS.last_apply_route() == "values_only"
        assert_same(a, cur, "borrowed, values only %d" % step)
        assert bufs[2].download(np.float32, len(val)).tobytes() == cur[4].tobytes()
    before = [buf.download(np.uint8, buf.nbytes) for buf in bufs]
    r = rng.integers(0, 520, 3000).astype(np.uint32)
    c = rng.integers(0, 320, 3000).astype(np.uint32)
    v = rng.uniform(-1, 1, 3000).astype(np.float32)
    a.apply(r, c, v)
    assert sm.SparseMatCRS.last_apply_route() == "general"
    assert_same(a, update_model.apply(cur, r, c, v), "borrowed, grows")
    after = [buf.download(np.uint8, buf.nbytes) for buf in bufs]
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_errors_leave_handle_untouched(gpu):
    rng = np.random.default_rng(41)
    m = rand(rng, 50, 40, 5, np.float32)
    a = dev(m)
    before = model_of(a)
    assert lib().smh_crs_apply(a._h, 3, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert lib().smh_crs_apply_dev(a._h, 3, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert lib().smh_crs_get_many(a._h, 3, None, None, None) == _lib.SMH_ERR_INVALID
    out = np.zeros(1, np.float32)
    assert lib().smh_crs_get(None, 0, 0, out.ctypes.data) == _lib.SMH_ERR_INVALID
    h = C.c_void_p()
    assert lib().smh_crs_eye(7, 3, C.byref(h)) == _lib.SMH_ERR_INVALID
    with pytest.raises(_lib.SparseMatPanic):
        a.apply([0], [0], np.ones(1, np.float64))  # values of the other dtype
    with pytest.raises(_lib.SparseMatPanic):
        a.add_to(2 ** 32 + 1, 0, 1.0)  # an index beyond u32 is refused, not truncated to 1
    with pytest.raises(_lib.SparseMatPanic):
        a.set(0, 2 ** 32, 1.0)
    assert_same(a, before, "untouched")
    n_dev = C.c_int()
    assert lib().smh_device_count(C.byref(n_dev)) == 0
    if n_dev.value < 2:
        pytest.skip("arrays on another device: needs two GPUs")
    assert lib().smh_set_device(1) == 0
    try:
        bufs = [upload(np.zeros(4, np.uint32)), upload(np.zeros(4, np.uint32)), upload(np.ones(4, np.float32))]
    finally:
        assert lib().smh_set_device(0) == 0
    assert lib().smh_crs_apply_dev(a._h, 4, C.c_void_p(bufs[0].ptr), C.c_void_p(bufs[1].ptr), C.c_void_p(bufs[2].ptr), None) == _lib.SMH_ERR_INVALID
    assert_same(a, before, "untouched after arrays on another device")


def test_get_many_at_scale(gpu):
    g = 128
    off, col, val = oracle.laplace3d(g, g, g, np.float32)
    n = g ** 3
    m = (n, n, off, col, val, 0)
    a = dev(m)
    rng = np.random.default_rng(51)
    q = 10_000_000
    r, c = existing_pairs(m, rng, q)
    kind = rng.random(q)
    c = np.where(kind < 0.2, rng.integers(0, n, q), c).astype(np.uint32)              # mostly absent
    r = np.where(kind > 0.95, rng.integers(n, n + 1000, q), r).astype(np.uint32)      # rows past the end
    want = update_model.get_many(m, r, c)
    assert a.get_many(r, c).tobytes() == want.tobytes()
    bufs = [upload(r), upload(c), DeviceBuffer(q * 4 + 16)]
    a.get_many_dev(q, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr)
    assert bufs[2].download(np.float32, q).tobytes() == want.tobytes()
    assert a.get(int(r[0]), int(c[0])).tobytes() == want[:1].tobytes()
