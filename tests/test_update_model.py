"""CPU: tests/update_model.py (the closed form of a set / add_to stream on a SparseMatCRS, SparseMatrix::get and ::eye) equals
the literal reference -- oracle.assembly.CrsPushMatrix seeded with m's arrays, then `set` / `add_to` per operation
(sparsematrix.rs:224-233, sparsemat_crs.rs:54-92) -- on random streams: interleaved set / add_to, repeated (row, column)
pairs, repeated columns in m, rows beyond m's, m with an orphan, m without rows, the recorded first push continued, signed
zeros and NaN."""
import numpy as np
import pytest

from oracle.assembly import CrsPushMatrix

import update_model
from test_add_model import random_crs


def seeded(m):
    """A CrsPushMatrix holding m (an orphan sits after the last row, where the quirk leaves it)."""
    m_rows, m_cols, m_off, m_col, m_val, m_orph = m
    dt = np.asarray(m_val).dtype.type
    c = CrsPushMatrix(dt)
    c.n_cols = m_cols
    if m_rows:
        c._n_rows = m_rows
        c.offset_rows = [int(v) for v in m_off[:m_rows + 1]]
    c.columns = [int(x) for x in m_col]
    c.values = [dt(v) for v in m_val]
    if m_orph:
        c.columns.append(0)
        c.values.append(dt(1.5))
    return c


def run_stream(c, rows, cols, vals, ops):
    for k in range(len(vals)):
        if ops is not None and ops[k]:
            c.set(int(rows[k]), int(cols[k]), vals[k])
        else:
            c.add_to(int(rows[k]), int(cols[k]), vals[k])
    return c


def state(c):
    dt = c.dtype
    n_rows = c.n_rows()
    off = np.array(c.offset_rows[:n_rows + 1] if n_rows else [0], np.uint32)
    nnz = int(off[-1])
    return (n_rows, c.n_cols, off, np.array(c.columns[:nnz], np.uint32), np.array(c.values[:nnz], dt), len(c.columns) - nnz)


def same(got, want, what=""):
    assert got[0] == want[0] and got[1] == want[1], (what, got[:2], want[:2])
    assert np.array_equal(got[2], want[2]), what
    assert np.array_equal(got[3], want[3]), what
    assert got[4].dtype == want[4].dtype and got[4].tobytes() == want[4].tobytes(), what
    assert got[5] == want[5], what


POOL = [0.0, -0.0, 1.0, -1.0, 0.5, 2.25, -3.75, 1e-3, 7.12, 1e30, np.nan]


def random_stream(rng, dtype, m, n_max=12, nan=True):
    n = int(rng.integers(1, n_max + 1))
    m_rows, m_cols = m[0], m[1]
    hi_r, hi_c = max(m_rows, 1) + 3, max(m_cols, 1) + 3
    rows = rng.integers(0, hi_r, n).astype(np.uint32)
    cols = rng.integers(0, hi_c, n).astype(np.uint32)
    if m[0] and m[3].size and rng.random() < 0.5:  # many operations on m's own entries (first occurrences and repeats)
        k = rng.integers(0, m[3].size, n)
        own = rng.random(n) < 0.7
        rows_m = np.repeat(np.arange(m_rows), np.diff(m[2].astype(np.int64)))
        rows[own] = rows_m[k[own]]
        cols[own] = m[3][k[own]]
    if n > 2 and rng.random() < 0.4:  # repeated (row, column) pairs in the stream
        j = rng.integers(0, n, n // 2)
        rows[j], cols[j] = rows[j[::-1]], cols[j[::-1]]
    pool = np.array(POOL if nan else POOL[:-1], dtype)
    vals = np.where(rng.random(n) < 0.5, pool[rng.integers(0, len(pool), n)], rng.uniform(-4, 4, n)).astype(dtype)
    ops = None if rng.random() < 0.25 else (rng.random(n) < 0.4).astype(np.uint8)
    return rows, cols, vals, ops


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_equals_literal_reference(dtype):
    rng = np.random.default_rng(20261017 + (dtype == np.float64))
    kinds = {"rows": 0, "orphan": 0, "new": 0, "recorded": 0}
    for case in range(1100):
        kind = case % 5
        first = None
        if kind == 3:  # SparseMatCRS::new()
            m = (0, int(rng.integers(0, 4)), np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype), 0)
            kinds["new"] += 1
        elif kind == 4:  # the state the first push leaves, with its record
            r0, c0, v0, op0 = int(rng.integers(0, 5)), int(rng.integers(0, 5)), dtype(rng.choice(POOL)), int(rng.integers(0, 2))
            first = update_model.first_op(r0, c0, v0, op0, dtype)
            m = (0, c0 + 1, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype), 1)
            kinds["recorded"] += 1
        else:
            m = random_crs(rng, dtype, allow_empty=False) + (int(kind == 2),)
            kinds["orphan" if kind == 2 else "rows"] += 1
        rows, cols, vals, ops = random_stream(rng, dtype, m)
        if first is not None:
            c = CrsPushMatrix(dtype)
            run_stream(c, [first[0]], [first[1]], [first[2]], [1])
        else:
            c = seeded(m)
        want = state(run_stream(c, rows, cols, vals, ops))
        got = update_model.apply(m, rows, cols, vals, ops, first=first)
        same(got, want, "case %d" % case)
    assert min(kinds.values()) > 100


def test_refused_without_record():
    m = (0, 3, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), 1)
    with pytest.raises(update_model.ApplyRefused):
        update_model.apply(m, [0], [0], np.ones(1, np.float32))


def test_signed_zero_and_set():
    m = (1, 1, np.array([0, 1], np.uint32), np.array([0], np.uint32), np.array([2.0], np.float32), 0)
    got = update_model.apply(m, [0, 0, 1, 2], [1, 2, 0, 0], np.array([-0.0, -0.0, 5, 6], np.float32), [0, 1, 0, 0])
    assert list(got[3]) == [2, 1, 0, 0, 0]
    assert np.signbit(got[4][0]) and not np.signbit(got[4][1])  # set(-0) keeps -0, add_to(-0) on a new entry gives +0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lookups_equal_literal_get(dtype):
    rng = np.random.default_rng(7 + (dtype == np.float64))
    for _ in range(200):
        m = random_crs(rng, dtype) + (0,)
        c = seeded(m)
        n = 20
        rows = rng.integers(0, m[0] + 3, n).astype(np.uint32)
        cols = rng.integers(0, m[1] + 2, n).astype(np.uint32)
        want = np.array([c.get(int(i), int(j)) for i, j in zip(rows, cols)], dtype)
        got = update_model.get_many(m, rows, cols)
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_eye_equals_literal(dtype):
    for dim in range(6):
        c = CrsPushMatrix(dtype)
        for i in range(dim):
            c.set(i, i, dtype(1))
        same(update_model.eye(dim, dtype), state(c), "dim %d" % dim)
