"""SparseMatrix::add / sub (sparsematrix.rs:123-143) of two SparseMatCRS, restated in vectorised numpy.

`a.add(&b)` runs `*a.get_mut(i, j) += val` for every entry of b in storage order.  On a SparseMatCRS with rows that
closed form is (checked against the literal oracle.assembly.CrsPushMatrix by tests/test_add_model.py):
  * n_rows = max(a.n_rows, 1 + last row of b holding an entry);
  * n_cols = max(a.n_cols, 1 + largest column that created a NEW entry);
  * row i = the new columns in REVERSE order of first appearance in b's row i (push prepends, sparsemat_crs.rs:85-87),
    then a's row i unchanged in order;
  * a b entry whose column exists in a's row folds into the FIRST occurrence (find_index :54-67); a new entry folds
    from zero; folds are sequential in b's storage order, one rounding per operation (acc + v, or acc - v for sub);
  * a's orphan stays; b's orphan is not visited.
a without rows and without an orphan is SparseMatCRS::new(): the result is the replay of b's stream (first-push quirk
included), n_cols at least a.n_cols.  a without rows but with an orphan is refused (its hidden offset_rows length
decides the outcome).

Matrices are tuples (n_rows, n_cols, offset_rows, columns, values, orphans); values carry the dtype.
"""
import numpy as np

import oracle


class AddRefused(ValueError):
    """a without rows but with an orphan: SMH_ERR_INVALID on the device."""


def _rows_of(off, n_rows):
    off = np.asarray(off, np.int64)
    return np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(off[:n_rows + 1]))


def add(a, b, subtract=False):
    """The SparseMatCRS `a` holds after `a.add(&b)` (`a.sub(&b)` with subtract=True)."""
    a_rows, a_cols, a_off, a_col, a_val, a_orph = a
    b_rows, b_cols, b_off, b_col, b_val = b[:5]
    dt = np.asarray(a_val).dtype
    a_off = np.asarray(a_off, np.uint32)
    b_off = np.asarray(b_off, np.uint32)
    nnz_a = int(a_off[a_rows]) if a_rows else 0
    nnz_b = int(b_off[b_rows]) if b_rows else 0
    a_col = np.asarray(a_col, np.uint32)[:nnz_a]
    a_val = np.asarray(a_val, dt)[:nnz_a]
    b_col = np.asarray(b_col, np.uint32)[:nnz_b]
    b_val = np.asarray(b_val, dt)[:nnz_b]
    if a_rows == 0:
        if a_orph:
            raise AddRefused("a has no rows but an orphaned entry")
        src = _rows_of(b_off, b_rows).astype(np.uint32)
        vals = -b_val if subtract else b_val
        n_rows, n_cols, off, col, val, stored = oracle.crs_replay(src, b_col, vals)
        return n_rows, max(n_cols, a_cols), off, col, val, stored - int(off[n_rows])

    rows_a = _rows_of(a_off, a_rows)
    rows_b = _rows_of(b_off, b_rows)
    n_rows = max(a_rows, int(rows_b[-1]) + 1 if nnz_b else 0)
    key_a = (rows_a.astype(np.uint64) << np.uint64(32)) | a_col.astype(np.uint64)
    key_b = (rows_b.astype(np.uint64) << np.uint64(32)) | b_col.astype(np.uint64)
    # first occurrence of every (row, column) of a
    u_a, first_a = np.unique(key_a, return_index=True)
    pos = np.searchsorted(u_a, key_b)
    hit = pos < len(u_a)
    hit[hit] = u_a[pos[hit]] == key_b[hit]
    target = np.empty(nnz_b, np.int64)
    target[hit] = first_a[pos[hit]]
    # new entries: first appearance of a (row, column) among the b entries that found nothing in a
    miss = np.flatnonzero(~hit)
    u_n, first_n, inv_n = np.unique(key_b[miss], return_index=True, return_inverse=True)
    new_k = miss[first_n]                       # b index of every new entry's first appearance
    order = np.argsort(new_k, kind="stable")    # new entries by first appearance (= row-major)
    new_id = np.empty(len(new_k), np.int64)
    new_id[order] = np.arange(len(new_k))
    target[miss] = nnz_a + new_id[inv_n.reshape(-1)]
    new_k = new_k[order]
    new_row = rows_b[new_k]
    cnt = np.bincount(new_row, minlength=n_rows).astype(np.int64)
    a_off_ext = np.full(n_rows + 1, nnz_a, np.int64)
    a_off_ext[:a_rows + 1] = a_off[:a_rows + 1]
    off = a_off_ext.copy()
    off[1:] += np.cumsum(cnt)
    # values: fold every target's b entries in storage order, one rank of repeats at a time
    acc = np.concatenate([a_val, np.zeros(len(new_k), dt)])
    by_t = np.lexsort((np.arange(nnz_b), target))
    t_sorted = target[by_t]
    starts = np.r_[True, t_sorted[1:] != t_sorted[:-1]] if nnz_b else np.zeros(0, bool)
    grp_start = np.maximum.accumulate(np.where(starts, np.arange(nnz_b), 0)) if nnz_b else np.zeros(0, np.int64)
    rank = np.arange(nnz_b) - grp_start
    for r in range(int(rank.max()) + 1 if nnz_b else 0):
        sel = by_t[rank == r]
        t = target[sel]
        acc[t] = (acc[t] - b_val[sel]) if subtract else (acc[t] + b_val[sel])
    # placement: new columns reversed, then a's row
    nnz = nnz_a + len(new_k)
    col = np.empty(nnz, np.uint32)
    val = np.empty(nnz, dt)
    row_first_new = np.searchsorted(new_row, np.arange(n_rows))
    rank_in_row = np.arange(len(new_k)) - row_first_new[new_row]
    p_new = off[new_row] + cnt[new_row] - 1 - rank_in_row
    col[p_new] = b_col[new_k]
    val[p_new] = acc[nnz_a:]
    p_a = off[rows_a] + cnt[rows_a] + (np.arange(nnz_a) - a_off_ext[rows_a])
    col[p_a] = a_col
    val[p_a] = acc[:nnz_a]
    n_cols = max(a_cols, int(b_col[new_k].max()) + 1 if len(new_k) else 0)
    return n_rows, n_cols, off.astype(np.uint32), col, val, a_orph
