"""What an update plan's execute leaves, restated through tests/update_model.py: without from_zero it is `apply` of the
stream; with from_zero it is `apply` of (one set(+0) per distinct (row, column) of the stream) ++ the stream -- pinned to the
literal reference by tests/test_update_plan_model.py."""
import numpy as np

import update_model


def zero_then_stream(rows, cols, vals, ops):
    """(one set(+0) per distinct pair) ++ the stream, as (rows, cols, vals, ops)."""
    rows = np.asarray(rows, np.uint32)
    cols = np.asarray(cols, np.uint32)
    vals = np.asarray(vals)
    n = len(vals)
    ops = np.zeros(n, np.uint8) if ops is None else np.asarray(ops, np.uint8)
    key = (rows.astype(np.uint64) << np.uint64(32)) | cols.astype(np.uint64)
    _, first = np.unique(key, return_index=True)
    return (np.r_[rows[first], rows].astype(np.uint32), np.r_[cols[first], cols].astype(np.uint32),
            np.r_[np.zeros(len(first), vals.dtype), vals].astype(vals.dtype), np.r_[np.ones(len(first), np.uint8), ops].astype(np.uint8))


def execute(m, rows, cols, vals, ops=None, from_zero=False):
    """The matrix tuple after plan.execute(vals, from_zero) of the plan made from (rows, cols, ops) on m."""
    if len(vals) == 0:
        return update_model.apply(m, rows, cols, vals, ops)
    if from_zero:
        rows, cols, vals, ops = zero_then_stream(rows, cols, np.asarray(vals, np.asarray(m[4]).dtype), ops)
    return update_model.apply(m, rows, cols, vals, ops)
