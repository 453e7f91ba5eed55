"""A reusable update plan on a device SparseMatCRS (csrc/matplan.hip): `plan.execute(values)` equals `apply` of the planned stream
bit for bit -- tests/plan_model.py over tests/update_model.py, pinned to the literal reference by test_update_plan_model.py --
for every run length around the kernels' thresholds, with `set`s anywhere in a run, from the stored values and from zero; the
plan is reusable, re-assembly reproduces assembly, derived forms follow the values, borrowed arrays are written in place, and
a plan is refused on another handle or once the structure changed."""
import ctypes as C

import numpy as np
import pytest

import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib, synth
from sparsemat_amd._lib import lib

import plan_model
from test_crs_add_gpu import assert_same, dev, model_of, rand
from test_crs_update_gpu import VARIANTS, _configured, existing_pairs, hex_stream, upload

pytestmark = pytest.mark.gpu


def make_plan(h, rows, cols, ops, form):
    if form == "host":
        return h.update_plan(rows, cols, ops), None
    bufs = [upload(np.asarray(rows, np.uint32)), upload(np.asarray(cols, np.uint32))]
    ob = None if ops is None else upload(np.asarray(ops, np.uint8))
    return h.update_plan_dev(len(rows), bufs[0].ptr, bufs[1].ptr, None if ob is None else ob.ptr), (bufs, ob)


def execute(plan, vals, from_zero, form):
    if form == "host":
        plan.execute(vals, from_zero)
    else:
        buf = upload(vals)
        plan.execute_dev(buf.ptr, from_zero)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_plan_equals_apply_and_is_reusable(gpu, dtype):
    rng = np.random.default_rng(211 + (dtype == np.float64))
    a = rand(rng, 300, 200, 9, dtype, dup=True)
    n = 5000
    rows, cols = existing_pairs(a, rng, n)
    values = []
    for _ in range(3):
        v = rng.uniform(-2, 2, n).astype(dtype)
        v[::7] = dtype(-0.0)
        v[::11] = np.nan
        values.append(v)
    for ops in ((rng.random(n) < 0.3).astype(np.uint8), None):
        for create_form in ("host", "dev"):
            for exec_form in ("host", "dev"):
                h = dev(a)
                plan, keep = make_plan(h, rows, cols, ops, create_form)
                assert plan.stats()["n_ops"] == n
                cur = a
                for step, (v, fz) in enumerate(zip(values, (False, True, False))):
                    execute(plan, v, fz, exec_form)
                    cur = plan_model.execute(cur, rows, cols, v, ops, fz)
                    assert_same(h, cur, "ops=%s create=%s execute=%s step %d" % (ops is not None, create_form, exec_form, step))
    # a handle that carries an orphan (the replay quirk)
    h = sm.SparseMatCRS.from_triplets([3, 1, 2], [1, 0, 2], np.array([1.5, 2.0, -1.0], dtype), into_crs=True)
    m = model_of(h)
    assert m[5] == 1 and m[0] > 0
    rows, cols = existing_pairs(m, rng, 40)
    ops = (rng.random(40) < 0.3).astype(np.uint8)
    plan = h.update_plan(rows, cols, ops)
    cur = m
    for fz in (False, True, False):
        v = rng.uniform(-2, 2, 40).astype(dtype)
        plan.execute(v, fz)
        cur = plan_model.execute(cur, rows, cols, v, ops, fz)
        assert_same(h, cur, "orphan-carrying handle, from_zero=%s" % fz)


RUN_MATRIX_ROWS, RUN_MATRIX_COLS = 6, 100
PLAN_STAGE = 2048  # operations the long-run kernel stages per round (csrc/matplan.hip: kPlanStage)
_run_stream_cache = {}


def run_length_stream(threshold):
    """One matrix of 6 rows x 100 distinct columns (plus short rows) and a stream, interleaved in stream order, of
    - one run of pure `add_to` per length around the kernels' switches: what is kept of them is all of them, so the long-run
      kernel meets runs that start from the stored value (or +0) at L + 1, 255 .. 257 and 5000 (more than two staging rounds);
    - further runs that carry the `set`s: at the first, a middle and the last position of short and long runs, runs of nothing
      but `set`s, long runs whose late `set` still keeps more than L operations (L + 1 exactly, and more than two rounds), and
      a run cut down to exactly L.
    Returns the kept length and `set` head of every run beside the stream."""
    if threshold in _run_stream_cache:
        return _run_stream_cache[threshold]
    rng = np.random.default_rng(77)
    lens_m = [RUN_MATRIX_COLS] * RUN_MATRIX_ROWS + [3] * 40
    off = np.zeros(len(lens_m) + 1, np.uint32)
    off[1:] = np.cumsum(lens_m)
    col = np.concatenate([rng.permutation(RUN_MATRIX_COLS)[:k] for k in lens_m]).astype(np.uint32)
    L = threshold
    pure = [1, 2, 3, 7, 8, 63, 64, 65, 255, 256, 257, L - 1, L, L + 1, 5000]
    # (run length, positions of its `set`s; None: every operation is a `set`)
    with_sets = [(5000, [0, 2500]),        # first and a middle position: 2500 kept, more than one round
                 (3 * PLAN_STAGE, [500]),  # a late-ish set that keeps more than two rounds
                 (257, [256]),             # last
                 (255, [0]),               # first: all kept
                 (256, [100]),             # middle: 156 kept
                 (L + 1, [L]),             # last of a run just over the threshold
                 (L + 11, [10]),           # keeps exactly L + 1, with a set head
                 (L + 10, [10]),           # keeps exactly L
                 (300, [200]),             # a late set that still keeps more than L
                 (7, [3]), (3, [2]), (8, [0]), (65, None), (2, None)]
    run_lens = pure + [n for n, _ in with_sets]
    targets = rng.permutation(int(off[-1]))[:len(run_lens)]  # distinct entries; every other entry has run length 0
    tid = rng.permutation(np.repeat(np.arange(len(run_lens)), run_lens))  # interleaved, not grouped
    ops = np.zeros(len(tid), np.uint8)
    where = [np.flatnonzero(tid == r) for r in range(len(run_lens))]
    for r, (_, sets) in enumerate(with_sets, len(pure)):
        ops[where[r] if sets is None else where[r][sets]] = 1
    rows_m = np.repeat(np.arange(len(lens_m), dtype=np.uint32), lens_m)
    rows, cols = rows_m[targets[tid]], col[targets[tid]]
    head_set = np.array([bool(ops[w].any()) for w in where])
    kept = np.array([len(w) - (np.flatnonzero(ops[w])[-1] if ops[w].any() else 0) for w in where])
    out = (off, col, rows, cols, ops, run_lens, kept, head_set)
    _run_stream_cache[threshold] = out
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_run_lengths_and_dead_operations(gpu, dtype):
    rng = np.random.default_rng(5 + (dtype == np.float64))
    probe = dev(rand(rng, 4, 4, 3, dtype))
    L = probe.update_plan([], []).stats()["long_run_threshold"]
    assert 1 < L < 5000
    off, col, rows, cols, ops, run_lens, kept, head_set = run_length_stream(L)
    n_targets, longest, live = len(run_lens), max(run_lens), int(kept.sum())
    # what the kernels see: both classes on both sides of the switch, the long one with and without a `set` head, from the
    # stored value over more than two staging rounds
    for want in (L - 1, L, L + 1):
        assert (kept[~head_set] == want).any(), want
    assert (kept[head_set] == L).any() and (kept[head_set] == L + 1).any()
    assert (kept[~head_set] > 2 * PLAN_STAGE).any() and (kept[head_set] > 2 * PLAN_STAGE).any()
    assert {65, 255, 256, 257, L + 1, 5000} <= set(kept[~head_set].tolist())
    assert ((kept > L) & head_set & (kept < np.array(run_lens))).any()  # a long run behind a dropped prefix
    val = rng.uniform(-1, 1, len(col)).astype(dtype)
    m = (len(off) - 1, RUN_MATRIX_COLS, off, col, val, 0)
    h = dev(m)
    plan = h.update_plan(rows, cols, ops)
    st = plan.stats()
    assert (st["n_ops"], st["n_targets"], st["longest_run"], st["n_live_ops"]) == (len(rows), n_targets, longest, live)
    assert st["device_bytes"] >= 4 * (st["n_live_ops"] + 2 * st["n_targets"])
    cur = m
    for fz in (False, True):
        v = rng.uniform(-1, 1, len(rows)).astype(dtype)
        v[::13] = dtype(-0.0)
        plan.execute(v, fz)
        cur = plan_model.execute(cur, rows, cols, v, ops, fz)
        assert_same(h, cur, "run lengths, from_zero=%s" % fz)
    # only sets: the last one of every pair is all that lives
    k = rng.permutation(len(col))[:100]
    rows_m = np.repeat(np.arange(m[0], dtype=np.uint32), np.diff(off.astype(np.int64)))
    order = rng.permutation(np.repeat(k, 50))
    r100, c100 = rows_m[order], col[order]
    plan2 = h.update_plan(r100, c100, np.ones(len(order), np.uint8))
    assert plan2.stats()["n_live_ops"] == 100 and plan2.stats()["n_targets"] == 100 and plan2.stats()["longest_run"] == 50
    v = rng.uniform(-1, 1, len(order)).astype(dtype)
    plan2.execute(v, True)
    cur = plan_model.execute(cur, r100, c100, v, np.ones(len(order), np.uint8), True)
    assert_same(h, cur, "only sets")


def test_long_rows_at_create(gpu):
    rng = np.random.default_rng(5)
    for max_len in (300, 5000):  # lookup by lane groups of 8, of 32
        lens = rng.integers(0, max_len + 1, 400)
        lens[0] = max_len
        off = np.zeros(len(lens) + 1, np.uint32)
        off[1:] = np.cumsum(lens)
        col = rng.integers(0, 20000, int(off[-1])).astype(np.uint32)
        col[1::5] = col[0:-1:5][:len(col[1::5])]  # duplicates: the first match is the target
        m = (len(lens), 20000, off, col, rng.uniform(-1, 1, len(col)).astype(np.float32), 0)
        rows, cols = existing_pairs(m, rng, 100_000)
        ops = (rng.random(len(rows)) < 0.2).astype(np.uint8)
        h = dev(m)
        plan = h.update_plan(rows, cols, ops)
        cur = m
        for fz in (False, True):
            v = rng.uniform(-1, 1, len(rows)).astype(np.float32)
            plan.execute(v, fz)
            cur = plan_model.execute(cur, rows, cols, v, ops, fz)
            assert_same(h, cur, "long rows %d, from_zero=%s" % (max_len, fz))


def test_reassembly_reproduces_assembly(gpu):
    rng = np.random.default_rng(3)
    rows, cols, v1 = hex_stream(24, np.float32, rng)
    assert len(rows) == 24 ** 3 * 64
    v2 = rng.uniform(-1, 1, len(rows)).astype(np.float32)
    m = sm.SparseMatCRS.from_triplets(rows, cols, v1)
    assembled = model_of(m)
    plan = m.update_plan(rows, cols)
    st = plan.stats()
    assert st["n_targets"] == assembled[2][-1] and st["n_live_ops"] == len(rows) and st["longest_run"] == 8
    m *= 3.0  # whatever is stored, from_zero does not read it
    plan.execute(v1, from_zero=True)
    assert_same(m, assembled, "re-assembly of the same stream")
    plan.execute(v2, from_zero=True)
    second = sm.SparseMatCRS.from_triplets(rows, cols, v2)
    assert_same(m, model_of(second), "re-assembly with new values")
    x = oracle.gen_x(synth.SEED_X, m.n_cols(), np.float32)
    for variant in ("auto", "seq"):
        assert m.mvp(x, variant=variant).tobytes() == second.mvp(x, variant=variant).tobytes(), variant


@pytest.mark.parametrize("shape", ["stencil", "stencil_many_values", "no_locality"])
def test_derived_forms_follow_the_values(gpu, shape):
    rng = np.random.default_rng(23)
    if shape != "no_locality":  # K1s direct codes; two distinct values: with the value dictionary
        g = 24
        off, col, val = oracle.laplace3d(g, g, g, np.float32)
        n = g ** 3
        if shape == "stencil_many_values":
            val = rng.uniform(-1, 1, len(val)).astype(np.float32)  # > 32 distinct values: no dictionary
    else:  # no column codes, so no dictionary whatever the values are; 1 % of the rows hold a quarter of the entries (K2s splits)
        n = 60_000
        lens = np.full(n, 8)
        lens[::100] = 300
        off = np.zeros(n + 1, np.uint32)
        off[1:] = np.cumsum(lens)
        within = np.arange(int(off[-1])) - np.repeat(off[:-1].astype(np.int64), lens)
        col = ((np.repeat(rng.integers(0, n, n), lens) + within * 7919) % n).astype(np.uint32)  # distinct inside a row
        val = rng.uniform(-1, 1, len(col)).astype(np.float32)
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
    assert set(ran) == set(VARIANTS), ran
    assert a.tiled_layout()["copy_entries"] >= len(col)  # K2t keeps a copy of the values
    if shape == "no_locality":  # ... and so do the row-length split and the fused column-blocked copy, where they are built
        assert a.colsplit_flag() and a.colfused(arrays=False)["fits"]
    dict_before = len(a.stream_value_dict()) > 0
    assert dict_before == (shape == "stencil")
    rows_m = np.repeat(np.arange(n, dtype=np.uint32), np.diff(off.astype(np.int64)))
    if dict_before:  # new values everywhere: the dictionary stops applying
        order = rng.permutation(len(col))
        plan = a.update_plan(rows_m[order], col[order])
        plan.execute(rng.uniform(-1, 1, len(col)).astype(np.float32), from_zero=True)
    else:  # every entry set to one of two values: the dictionary applies afterwards, where the columns allow one
        plan = a.update_plan(rows_m, col, np.ones(len(col), np.uint8))
        plan.execute(np.where(col == rows_m, 4.0, -1.0).astype(np.float32))
    g_off, g_col, g_val = a.raw_parts()
    assert g_val.tobytes() != val.tobytes()
    fresh = _configured(n, g_off, g_col, g_val)
    for v in ran:
        assert a.mvp(x, variant=v).tobytes() == fresh.mvp(x, variant=v).tobytes(), v
    assert (len(a.stream_value_dict()) > 0) == (shape == "stencil_many_values")
    assert a.stream_value_dict().tobytes() == fresh.stream_value_dict().tobytes()


def test_borrowed_arrays(gpu):
    rng = np.random.default_rng(31)
    m = rand(rng, 500, 300, 7, np.float32, dup=True)
    n_rows, n_cols, off, col, val, _ = m
    bufs = [upload(a) for a in (off, col, val)]
    a = sm.SparseMatCRS.from_device_parts(n_rows, n_cols, len(val), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, np.float32, keep=bufs)
    rows, cols = existing_pairs(m, rng, 3000)
    plan = a.update_plan(rows, cols)
    cur = m
    for fz in (False, True):  # written into the lent array, still borrowing
        v = rng.uniform(-1, 1, 3000).astype(np.float32)
        plan.execute(v, fz)
        cur = plan_model.execute(cur, rows, cols, v, None, fz)
        assert_same(a, cur, "borrowed, from_zero=%s" % fz)
        assert bufs[2].download(np.float32, len(val)).tobytes() == cur[4].tobytes()
    assert bufs[0].download(np.uint32, len(off)).tobytes() == off.tobytes()
    assert bufs[1].download(np.uint32, len(col)).tobytes() == col.tobytes()


def _absent_pair(m):
    n_rows, n_cols, off, col = m[:4]
    for i in range(n_rows):
        free = np.setdiff1d(np.arange(n_cols, dtype=np.uint32), col[off[i]:off[i + 1]])
        if len(free):
            return i, int(free[0])
    raise AssertionError("the matrix is full")


def test_staleness_and_errors(gpu):
    rng = np.random.default_rng(41)
    m = rand(rng, 50, 40, 5, np.float32)
    rows, cols = existing_pairs(m, rng, 300)
    vals = rng.uniform(-1, 1, 300).astype(np.float32)
    ai, aj = _absent_pair(m)
    # create: one absent pair is refused with the count, m untouched
    a = dev(m)
    with pytest.raises(_lib.SparseMatPanic) as e:
        a.update_plan(np.r_[rows, np.uint32(ai)], np.r_[cols, np.uint32(aj)])
    assert e.value.status == _lib.SMH_ERR_INVALID and " 1 of 301 " in str(e.value)
    assert_same(a, m, "create refused")
    h = C.c_void_p(1)
    assert lib().smh_update_plan_create(a._h, 3, None, None, None, C.byref(h)) == _lib.SMH_ERR_INVALID and not h.value
    assert lib().smh_update_plan_create_dev(a._h, 3, None, None, None, C.byref(h)) == _lib.SMH_ERR_INVALID
    with pytest.raises(_lib.SparseMatPanic) as e:
        sm.SparseMatCRS.new(np.float32).update_plan([0], [0])
    assert e.value.status == _lib.SMH_ERR_INVALID
    # execute succeeds after everything that leaves the structure alone
    plan = a.update_plan(rows, cols)
    other = a.update_plan(rows[::-1].copy(), cols[::-1].copy(), np.ones(300, np.uint8))
    cur = m
    a *= 0.5
    cur = cur[:4] + ((cur[4] * np.float32(0.5)).astype(np.float32), 0)
    plan.execute(vals)
    cur = plan_model.execute(cur, rows, cols, vals)
    assert_same(a, cur, "after scale")
    a.update_values(m[4])
    plan.execute(vals, True)
    cur = plan_model.execute(m, rows, cols, vals, None, True)
    assert_same(a, cur, "after update_values")
    a.apply(rows[:50], cols[:50], vals[:50])
    assert sm.SparseMatCRS.last_apply_route() == "values_only"
    other.execute(vals)
    a += dev(cur)  # the same pattern: the values-only route of +=
    assert sm.SparseMatCRS.last_add_route() != "general"
    before = model_of(a)
    plan.execute(vals)
    assert_same(a, plan_model.execute(before, rows, cols, vals), "after values-only apply, the other plan and a values-only +=")
    assert lib().smh_update_plan_execute(plan._h, a._h, None, 0) == _lib.SMH_ERR_INVALID
    assert lib().smh_update_plan_execute_dev(plan._h, a._h, None, 0) == _lib.SMH_ERR_INVALID
    # execute is refused, m untouched, once the structure changed or on another handle

    def refused(matrix, p, what):
        before = model_of(matrix)
        assert lib().smh_update_plan_execute(p._h, matrix._h, vals.ctypes.data, 0) == _lib.SMH_ERR_INVALID, what
        buf = upload(vals)
        assert lib().smh_update_plan_execute_dev(p._h, matrix._h, C.c_void_p(buf.ptr), 1) == _lib.SMH_ERR_INVALID, what
        assert_same(matrix, before, what)

    b = dev(m)
    p = b.update_plan(rows, cols)
    b.sort_rows()
    refused(b, p, "after sort_rows")
    b = dev(m)
    p = b.update_plan(rows, cols)
    b.apply([ai], [aj], np.ones(1, np.float32))
    assert sm.SparseMatCRS.last_apply_route() == "general"
    refused(b, p, "after an apply that added an entry")
    b.update_plan(rows, cols).execute(vals)  # a new plan on the new structure works
    b = dev(m)
    p = b.update_plan(rows, cols)
    one = np.zeros(m[0] + 1, np.uint32)
    one[ai + 1:] = 1
    b += sm.SparseMatCRS.from_raw_parts(m[0], m[1], one, np.array([aj], np.uint32), np.ones(1, np.float32))
    assert b.n_non_zero_entries() == len(m[3]) + 1
    refused(b, p, "after += with a new entry")
    b = dev(m)
    p = b.update_plan(rows, cols)
    refused(b.clone(), p, "on a clone")
    p.execute(vals)  # still valid on its own handle
    # an empty plan executes as a no-op
    empty = b.update_plan([], [])
    assert empty.stats()["n_ops"] == 0 and empty.stats()["n_targets"] == 0
    before = model_of(b)
    empty.execute(np.zeros(0, np.float32), True)
    empty.execute_dev(None)
    assert_same(b, before, "empty plan")
    # a plan may outlive its matrix: it can then only be destroyed
    d = dev(m)
    raw = C.c_void_p()
    r32, c32 = np.ascontiguousarray(rows, np.uint32), np.ascontiguousarray(cols, np.uint32)
    assert lib().smh_update_plan_create(d._h, len(r32), r32.ctypes.data, c32.ctypes.data, None, C.byref(raw)) == 0
    del d
    assert lib().smh_update_plan_destroy(raw) == 0
    assert lib().smh_update_plan_destroy(None) == 0
