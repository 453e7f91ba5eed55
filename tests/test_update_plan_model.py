"""CPU: the restatement of an update plan's from_zero execute (tests/plan_model.py: one set(+0) per distinct (row, column) of the
stream, then the stream) equals the literal reference -- oracle.assembly.CrsPushMatrix seeded with m, its targeted values
overwritten with +0, then `set` / `add_to` per operation -- on random streams of existing pairs: interleaved set / add_to,
repeated pairs, repeated columns inside a row of m (the first match is the target), signed zeros and NaN."""
import numpy as np
import pytest

import plan_model
import update_model
from test_add_model import random_crs
from test_update_model import random_stream, run_stream, same, seeded, state


def existing_only(m, rows, cols, vals, ops):
    n_rows, _, off, col = m[:4]
    rows_m = np.repeat(np.arange(n_rows, dtype=np.uint64), np.diff(off.astype(np.int64)))
    key_m = (rows_m << np.uint64(32)) | col.astype(np.uint64)
    key_s = (rows.astype(np.uint64) << np.uint64(32)) | cols.astype(np.uint64)
    keep = np.isin(key_s, key_m)
    return rows[keep], cols[keep], vals[keep], None if ops is None else ops[keep]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_from_zero_restatement_equals_literal_reference(dtype):
    rng = np.random.default_rng(20261018 + (dtype == np.float64))
    seen = {"cases": 0, "nan": 0, "neg_zero": 0, "dup_column_targeted": 0, "sets": 0, "untargeted_kept": 0}
    while seen["cases"] < 500:
        m = random_crs(rng, dtype, allow_empty=False) + (0,)
        rows, cols, vals, ops = existing_only(m, *random_stream(rng, dtype, m, n_max=24))
        if len(vals) == 0:
            continue
        seen["cases"] += 1
        c = seeded(m)
        targeted = {c._find_index(int(i), int(j)) for i, j in zip(rows, cols)}
        assert None not in targeted
        for k in targeted:
            c.values[k] = dtype(0.0)
        want = state(run_stream(c, rows, cols, vals, ops))
        got = plan_model.execute(m, rows, cols, vals, ops, from_zero=True)
        same(got, want, "case %d" % seen["cases"])
        # without from_zero the plan is apply itself
        same(plan_model.execute(m, rows, cols, vals, ops), state(run_stream(seeded(m), rows, cols, vals, ops)))
        seen["nan"] += bool(np.isnan(vals).any())
        seen["neg_zero"] += bool((np.signbit(vals) & (vals == 0)).any())
        seen["sets"] += bool(ops is not None and ops.any())
        seen["untargeted_kept"] += len(targeted) < len(m[3])
        for i, j in zip(rows, cols):
            s, e = int(m[2][i]), int(m[2][i + 1])
            if np.count_nonzero(m[3][s:e] == j) > 1:
                seen["dup_column_targeted"] += 1
                break
    assert min(seen.values()) >= 50, seen


def test_from_zero_signed_zero():
    """set(+0) then add_to(-0.0) gives +0 (0 + -0 = +0), then a set(-0.0) keeps -0; an untargeted entry keeps its value."""
    m = (1, 3, np.array([0, 3], np.uint32), np.array([0, 1, 2], np.uint32), np.array([5.0, 6.0, 7.0], np.float32), 0)
    got = plan_model.execute(m, [0, 0], [0, 1], np.array([-0.0, -0.0], np.float32), [0, 1], from_zero=True)
    assert not np.signbit(got[4][0]) and got[4][0] == 0 and np.signbit(got[4][1]) and got[4][2] == 7.0
