"""A stream of SparseMatrix::set / add_to calls (sparsematrix.rs:224-233) on a SparseMatCRS, restated in vectorised numpy,
plus SparseMatrix::get (sparsemat_crs.rs:136-142) and SparseMatrix::eye (sparsematrix.rs:91-98).

`m.add_to(i, j, v)` is `*m.get_mut(i, j) += v`, `m.set(i, j, v)` is `*m.get_mut(i, j) = v`; get_mut finds the FIRST match
in row i or else pushes at the START of the row.  On a SparseMatCRS with rows the whole stream has a closed form (checked
against the literal oracle.assembly.CrsPushMatrix by tests/test_update_model.py) -- tests/add_model.py's form with b's entries
replaced by a stream in any row order, `set` mixed in:
  * n_rows = max(m.n_rows, 1 + largest row of any operation);
  * n_cols = max(m.n_cols, 1 + largest column that created a NEW entry);
  * row i = its new columns in REVERSE order of first appearance among the stream's operations on row i, then m's row i;
  * an operation whose (row, column) exists in m's row goes to the first occurrence;
  * every target is the left fold of its operations in stream order, from m's value or +0 (add_to: acc + v, set: v);
  * m's orphan stays.
m without rows: the replay of the stream (first-push quirk included), n_cols at least m.n_cols; with an orphan, the replay of
(its recorded first operation ++ the stream), refused without the record.

Matrices are tuples (n_rows, n_cols, offset_rows, columns, values, orphans); values carry the dtype.  A recorded first
operation is (row, column, folded value) -- see first_op().
"""
import numpy as np

import oracle


class ApplyRefused(ValueError):
    """m without rows, with an orphan but without its recorded operation: SMH_ERR_INVALID on the device."""


def _rows_of(off, n_rows):
    off = np.asarray(off, np.int64)
    return np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(off[:n_rows + 1]))


def first_op(row, col, val, op, dtype):
    """The record a one-operation replay keeps: push(i, j, zero) then `=` (op 1) or `+=` (op 0)."""
    v = dtype(val) if op else dtype(dtype(0) + dtype(val))
    return int(row), int(col), v


def apply(m, rows, cols, vals, ops=None, first=None):
    """The SparseMatCRS `m` holds after the stream (ops[k] == 1: set, else add_to); `first` = m's recorded first operation."""
    m_rows, m_cols, m_off, m_col, m_val, m_orph = m
    dt = np.asarray(m_val).dtype
    rows = np.asarray(rows, np.uint32)
    cols = np.asarray(cols, np.uint32)
    vals = np.asarray(vals, dt)
    n = len(vals)
    ops = np.zeros(n, np.uint8) if ops is None else np.asarray(ops, np.uint8)
    m_off = np.asarray(m_off, np.uint32)
    nnz_m = int(m_off[m_rows]) if m_rows else 0
    m_col = np.asarray(m_col, np.uint32)[:nnz_m]
    m_val = np.asarray(m_val, dt)[:nnz_m]
    if n == 0:
        return m_rows, m_cols, m_off[:m_rows + 1] if m_rows else np.zeros(1, np.uint32), m_col, m_val, m_orph
    if m_rows == 0:
        if m_orph:
            if first is None:
                raise ApplyRefused("m has no rows but an orphaned entry without its operation")
            rows = np.r_[np.uint32(first[0]), rows].astype(np.uint32)
            cols = np.r_[np.uint32(first[1]), cols].astype(np.uint32)
            vals = np.r_[np.asarray([first[2]], dt), vals].astype(dt)
            ops = np.r_[np.uint8(1), ops].astype(np.uint8)
        n_rows, n_cols, off, col, val, stored = oracle.crs_replay(rows, cols, vals, ops)
        return n_rows, max(n_cols, m_cols), off, col, val, stored - int(off[n_rows])

    rows_m = _rows_of(m_off, m_rows)
    r64 = rows.astype(np.int64)
    n_rows = max(m_rows, int(r64.max()) + 1)
    key_m = (rows_m.astype(np.uint64) << np.uint64(32)) | m_col.astype(np.uint64)
    key_s = (rows.astype(np.uint64) << np.uint64(32)) | cols.astype(np.uint64)
    u_m, first_m = np.unique(key_m, return_index=True)  # first occurrence of every (row, column) of m
    pos = np.searchsorted(u_m, key_s)
    hit = pos < len(u_m)
    hit[hit] = u_m[pos[hit]] == key_s[hit]
    target = np.empty(n, np.int64)
    target[hit] = first_m[pos[hit]]
    # new entries: first appearance of a (row, column) among the operations that found nothing in m
    miss = np.flatnonzero(~hit)
    u_n, first_n, inv_n = np.unique(key_s[miss], return_index=True, return_inverse=True)
    new_k = miss[first_n]                                 # stream position of every new entry's first appearance
    order = np.lexsort((new_k, r64[new_k]))               # row-major, by first appearance inside the row
    new_id = np.empty(len(new_k), np.int64)
    new_id[order] = np.arange(len(new_k))
    target[miss] = nnz_m + new_id[inv_n.reshape(-1)]
    new_k = new_k[order]
    new_row = r64[new_k]
    cnt = np.bincount(new_row, minlength=n_rows).astype(np.int64)
    m_off_ext = np.full(n_rows + 1, nnz_m, np.int64)
    m_off_ext[:m_rows + 1] = m_off[:m_rows + 1]
    off = m_off_ext.copy()
    off[1:] += np.cumsum(cnt)
    # values: fold every target's operations in stream order, one rank of repeats at a time
    acc = np.concatenate([m_val, np.zeros(len(new_k), dt)])
    by_t = np.lexsort((np.arange(n), target))
    t_sorted = target[by_t]
    starts = np.r_[True, t_sorted[1:] != t_sorted[:-1]]
    grp_start = np.maximum.accumulate(np.where(starts, np.arange(n), 0))
    rank = np.arange(n) - grp_start
    for r in range(int(rank.max()) + 1):
        sel = by_t[rank == r]
        t = target[sel]
        acc[t] = np.where(ops[sel] != 0, vals[sel], acc[t] + vals[sel])
    # placement: new columns reversed, then m's row
    nnz = nnz_m + len(new_k)
    col = np.empty(nnz, np.uint32)
    val = np.empty(nnz, dt)
    row_first_new = np.searchsorted(new_row, np.arange(n_rows))
    rank_in_row = np.arange(len(new_k)) - row_first_new[new_row]
    p_new = off[new_row] + cnt[new_row] - 1 - rank_in_row
    col[p_new] = cols[new_k]
    val[p_new] = acc[nnz_m:]
    p_m = off[rows_m] + cnt[rows_m] + (np.arange(nnz_m) - m_off_ext[rows_m])
    col[p_m] = m_col
    val[p_m] = acc[:nnz_m]
    n_cols = max(m_cols, int(cols[new_k].max()) + 1 if len(new_k) else 0)
    return n_rows, n_cols, off.astype(np.uint32), col, val, m_orph


def get_many(m, rows, cols):
    """SparseMatrix::get for every (rows[k], cols[k]): the first match in the row, +0 when absent or rows[k] >= n_rows."""
    m_rows, _, m_off, m_col, m_val = m[:5]
    dt = np.asarray(m_val).dtype
    rows = np.asarray(rows, np.uint32)
    cols = np.asarray(cols, np.uint32)
    out = np.zeros(len(rows), dt)
    if m_rows == 0 or len(rows) == 0:
        return out
    m_off = np.asarray(m_off, np.uint32)
    nnz_m = int(m_off[m_rows])
    rows_m = _rows_of(m_off, m_rows)
    key_m = (rows_m.astype(np.uint64) << np.uint64(32)) | np.asarray(m_col, np.uint64)[:nnz_m]
    key_q = (rows.astype(np.uint64) << np.uint64(32)) | cols.astype(np.uint64)
    u_m, first_m = np.unique(key_m, return_index=True)
    pos = np.searchsorted(u_m, key_q)
    hit = pos < len(u_m)
    hit[hit] = u_m[pos[hit]] == key_q[hit]
    out[hit] = np.asarray(m_val, dt)[first_m[pos[hit]]]
    return out


def eye(dim, dtype):
    """SparseMatrix::eye on a SparseMatCRS: set(i, i, 1) for i < dim (dim 1: no rows, one orphan, n_cols 1)."""
    if dim == 0:
        return 0, 0, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype), 0
    if dim == 1:
        return 0, 1, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype), 1
    return dim, dim, np.arange(dim + 1, dtype=np.uint32), np.arange(dim, dtype=np.uint32), np.ones(dim, dtype), 0
