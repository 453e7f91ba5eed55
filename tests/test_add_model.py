"""CPU: tests/add_model.py (the closed form of SparseMatrix::add / sub on SparseMatCRS operands) equals the literal
reference -- oracle.assembly.CrsPushMatrix seeded with a's arrays, then `*get_mut(i, j) += val` (or -=) for every
entry of b in storage order (sparsematrix.rs:123-143, sparsemat_crs.rs:54-92) -- and holds the reference's own known
answers (src/lib.rs:74-79, :104-107)."""
import json
import os

import numpy as np
import pytest

from oracle.assembly import CrsPushMatrix, IndexListMatrix

import add_model

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")


def literal(a, b, subtract=False):
    """The reference's loop on a CrsPushMatrix holding a (an orphan sits after the last row, where the quirk leaves it)."""
    a_rows, a_cols, a_off, a_col, a_val, a_orph = a
    b_rows, b_cols, b_off, b_col, b_val = b[:5]
    dt = np.asarray(a_val).dtype.type
    m = CrsPushMatrix(dt)
    m.n_cols = a_cols
    if a_rows:
        m._n_rows = a_rows
        m.offset_rows = [int(v) for v in a_off[:a_rows + 1]]
    m.columns = [int(c) for c in a_col]
    m.values = [dt(v) for v in a_val]
    if a_orph:
        m.columns.append(0)
        m.values.append(dt(1.5))
    for i in range(b_rows):
        for k in range(int(b_off[i]), int(b_off[i + 1])):
            e = m._get_mut(i, int(b_col[k]))
            m.values[e] = dt(m.values[e] - b_val[k]) if subtract else dt(m.values[e] + b_val[k])
    n_rows = m.n_rows()
    off = np.array(m.offset_rows[:n_rows + 1] if n_rows else [0], np.uint32)
    nnz = int(off[-1])
    return (n_rows, m.n_cols, off, np.array(m.columns[:nnz], np.uint32), np.array(m.values[:nnz], dt),
            len(m.columns) - nnz)


def random_crs(rng, dtype, max_rows=6, max_cols=6, max_len=5, allow_empty=True):
    n_rows = int(rng.integers(0 if allow_empty else 1, max_rows + 1))
    n_cols = int(rng.integers(1, max_cols + 1))
    lens = rng.integers(0, max_len + 1, n_rows)
    if n_rows and rng.random() < 0.3:
        lens[-int(rng.integers(1, n_rows + 1)):] = 0  # trailing empty rows
    off = np.zeros(n_rows + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    nnz = int(off[-1])
    col = rng.integers(0, n_cols, nnz).astype(np.uint32)  # repeats inside a row included
    pool = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.25, -3.75, 1e-3, 7.12, 1e30], dtype)
    val = np.where(rng.random(nnz) < 0.5, pool[rng.integers(0, len(pool), nnz)], rng.uniform(-4, 4, nnz)).astype(dtype)
    return n_rows, n_cols, off, col, val


def same(got, want):
    assert got[0] == want[0] and got[1] == want[1], (got[:2], want[:2])
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[3], want[3])
    assert got[4].dtype == want[4].dtype and got[4].tobytes() == want[4].tobytes()
    assert got[5] == want[5]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_equals_literal_reference(dtype):
    rng = np.random.default_rng(20261016 + (dtype == np.float64))
    refused = replayed = grown = 0
    for case in range(1100):
        a = random_crs(rng, dtype) + (int(rng.random() < 0.15),)
        if case % 7 == 0:  # b on a's pattern (cancellations, repeats landing on the first occurrence)
            b = (a[0], a[1], a[2], a[3].copy(), (a[4] * dtype(rng.choice([1, -1, 0.5]))).astype(dtype))
        elif case % 7 == 1:  # b larger than a
            b = random_crs(rng, dtype, max_rows=9, max_cols=9)
        else:
            b = random_crs(rng, dtype)
        sub = bool(rng.random() < 0.5)
        want = literal(a, b, sub)
        if a[0] == 0 and a[5]:
            refused += 1
            with pytest.raises(add_model.AddRefused):
                add_model.add(a, b, sub)
            continue
        got = add_model.add(a, b, sub)
        replayed += a[0] == 0
        grown += got[0] > a[0] or got[1] > a[1]
        same(got, want)
    assert refused and replayed and grown


def test_model_without_rows_is_the_replay():
    """a = SparseMatCRS::new(): the result is oracle.crs_replay of b's stream, first-push quirk and orphan included."""
    f32 = np.float32
    empty = (0, 7, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, f32), 0)
    # row 2 then row 2: both pushed to the row's start -> the later first
    b = (3, 4, np.array([0, 0, 0, 2], np.uint32), np.array([3, 1], np.uint32), np.array([1.0, 2.0], f32))
    got = add_model.add(empty, b, subtract=True)
    assert got[0] == 3 and got[1] == 7 and got[5] == 0
    assert got[3].tolist() == [1, 3] and got[4].tolist() == [-2.0, -1.0]
    same(got, literal(empty, b, True))
    # the same (row, column) twice: the quirk leaves the first push an entry of its own at the end of the row
    b = (1, 4, np.array([0, 2], np.uint32), np.array([3, 3], np.uint32), np.array([1.0, 2.0], f32))
    got = add_model.add(empty, b)
    assert got[3].tolist() == [3, 3] and got[4].tolist() == [2.0, 1.0]
    same(got, literal(empty, b))
    # a single entry: no rows, one orphan
    b = (2, 4, np.array([0, 0, 1], np.uint32), np.array([2], np.uint32), np.array([1.0], f32))
    got = add_model.add(empty, b)
    assert got[0] == 0 and got[5] == 1
    same(got, literal(empty, b))


def _kat_sp():
    case = json.load(open(GOLDEN))["cases"][0]
    m = IndexListMatrix(np.float32)
    for op, i, j, v in case["ops"]:
        getattr(m, op)(i, j, np.float32(v))
    n_rows, n_cols, off, col, val = m.to_crs_arrays()
    return (n_rows, n_cols, off, col, val, 0)


def _get(m, i, j):
    off, col, val = m[2], m[3], m[4]
    for k in range(int(off[i]), int(off[i + 1])):
        if col[k] == j:
            return val[k]
    return m[4].dtype.type(0)


def test_reference_known_answers():
    sp = _kat_sp()
    ssum = add_model.add(sp, sp)
    assert _get(ssum, 0, 0) == np.float32(14.24)                      # lib.rs:74-75
    diff = add_model.add(ssum, sp, subtract=True)
    assert _get(diff, 0, 0) == _get(sp, 0, 0)                         # :76-77
    scaled = (sp[4] * np.float32(2.0)).astype(np.float32)             # Mul<T> = clone + scale (sparsematrix.rs:422-432)
    assert scaled[np.flatnonzero(sp[3][:sp[2][1]] == 0)[0]] == _get(ssum, 0, 0)  # :78-79
    assert [float(_get(ssum, 1, j)) for j in range(3)] == [0.0, float(np.float32(4.48)), float(np.float32(8.24))]  # :104-107
    same(ssum, literal(sp, sp))
