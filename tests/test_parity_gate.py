"""The SpMV parity gate itself (tests/util.py::assert_spmv_close) on the CPU: what it must refuse and what it must let through.
The gate stands behind every comparison of a kernel that is not bit-exact by construction, so a result it cannot tell from the
oracle's is a result the suite cannot see -- an all-NaN y passed it once (every test was "bad where err > bound")."""
import json

import numpy as np
import pytest

import oracle
import util
from util import PARITY_STATS, REL_TOL, assert_spmv_close, random_crs

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


@pytest.fixture(autouse=True)
def _keep_the_suite_statistics(monkeypatch):
    """These tests feed the gate results of their own making: the totals the suite prints at its end are put back, and the
    bucket records stay out of the suite's log file (they are still printed)."""
    saved = dict(PARITY_STATS, worst_literal=dict(PARITY_STATS["worst_literal"]))
    monkeypatch.setattr(util, "BUCKET_LOG_FILE", False)
    yield
    PARITY_STATS.clear()
    PARITY_STATS.update(saved)


def _matrix(dtype):
    rng = np.random.default_rng(300200)
    n_rows, n_cols = 300, 200
    lens = rng.integers(0, 12, n_rows)
    lens[7] = 0  # (an empty row at a known place)
    lens[8] = 9
    off, col, val = random_crs(rng, n_rows, n_cols, lens, dtype, dup=True)
    x = rng.uniform(-1, 1, n_cols).astype(dtype)
    return off, col, val, x, lens


def _refused(y, off, col, val, x):
    with pytest.raises(AssertionError):
        assert_spmv_close(y, off, col, val, x, "gate")


@DTYPES
def test_gate_passes_the_oracle_and_a_one_ulp_move(dtype):
    off, col, val, x, lens = _matrix(dtype)
    y = oracle.spmv(off, col, val, x)
    before = dict(PARITY_STATS, worst_literal=dict(PARITY_STATS["worst_literal"]))
    assert np.array_equal(assert_spmv_close(y.copy(), off, col, val, x, "oracle"), y)
    assert PARITY_STATS["comparisons"] == before["comparisons"] + 1 and PARITY_STATS["rows"] == before["rows"] + 300
    assert PARITY_STATS["fallback_rows"] == before["fallback_rows"] and PARITY_STATS["nonfinite_rows"] == before["nonfinite_rows"]
    for direction in (np.inf, -np.inf):
        moved = np.nextafter(y, dtype(direction))
        assert (moved != y).all()
        assert_spmv_close(moved, off, col, val, x, "one ulp")
    assert PARITY_STATS["worst_literal"][np.dtype(dtype).name] > 0.0


@DTYPES
def test_gate_refuses_nan_and_inf_where_the_oracle_is_finite(dtype):
    off, col, val, x, lens = _matrix(dtype)
    y = oracle.spmv(off, col, val, x)
    assert np.isfinite(y).all() and lens[7] == 0 and lens[8] > 0 and y[7] == 0
    _refused(np.full(len(y), np.nan, dtype), off, col, val, x)
    for row in (8, 7):  # a non-empty row, an empty one
        bad = y.copy()
        bad[row] = np.nan
        _refused(bad, off, col, val, x)
    for row in (8, 7):
        bad = y.copy()
        bad[row] = np.inf
        _refused(bad, off, col, val, x)
    # a NaN in the LAST row, and NaN everywhere but one row (nothing in the gate may be a reduction that skips NaN)
    bad = y.copy()
    bad[-1] = np.nan
    _refused(bad, off, col, val, x)
    bad = np.full(len(y), np.nan, dtype)
    bad[8] = y[8]
    _refused(bad, off, col, val, x)


@DTYPES
def test_gate_refuses_a_row_off_by_twice_the_tolerance(dtype):
    off, col, val, x, lens = _matrix(dtype)
    y = oracle.spmv(off, col, val, x)
    scale = oracle.spmv_abs(off, col, val, x)
    tol = REL_TOL[np.dtype(dtype)]
    for row in (8, int(np.argmax(lens))):
        for sign in (1.0, -1.0):
            bad = y.copy()
            bad[row] = dtype(float(y[row]) + sign * 2 * tol * scale[row])
            assert abs(float(bad[row]) - float(y[row])) > 1.5 * tol * scale[row]  # (the move survived the rounding to dtype)
            _refused(bad, off, col, val, x)
        ok = y.copy()
        ok[row] = dtype(float(y[row]) + 0.5 * tol * scale[row])
        assert_spmv_close(ok, off, col, val, x, "half the tolerance")


@DTYPES
def test_gate_compares_non_finite_oracle_rows_by_class(dtype):
    off, col, val, x, lens = _matrix(dtype)
    val = np.abs(val) + dtype(0.25)         # all values positive: Inf in x gives +Inf, -Inf gives -Inf, both give NaN
    x = x.copy()
    cols8 = col[off[8]:off[9]]
    x[cols8[0]] = np.inf
    rows_inf = [i for i in range(300) if (col[off[i]:off[i + 1]] == cols8[0]).any()]
    free = np.setdiff1d(np.arange(200), np.unique(np.concatenate([col[off[i]:off[i + 1]] for i in rows_inf])))
    x[free[0]] = np.nan
    x[free[1]] = -np.inf
    y = oracle.spmv(off, col, val, x)
    cls = util.value_class(y)
    i_pinf, i_nan, i_ninf = (int(np.nonzero(cls == c)[0][0]) for c in (1, 3, 2))
    assert 8 in rows_inf and cls[8] == 1 and (cls == 0).sum() > 100
    before = PARITY_STATS["nonfinite_rows"]
    assert_spmv_close(y.copy(), off, col, val, x, "non-finite x")
    assert PARITY_STATS["nonfinite_rows"] == before + int((cls != 0).sum())
    # NaN sign and payload are not part of the contract
    other = y.copy()
    u = np.uint32 if dtype == np.float32 else np.uint64
    other.view(u)[i_nan] ^= u(1) << u(31 if dtype == np.float32 else 63)
    other.view(u)[i_nan] |= u(5)
    assert np.isnan(other[i_nan]) and other.view(u)[i_nan] != y.view(u)[i_nan]
    assert_spmv_close(other, off, col, val, x, "another NaN")
    for row, wrong in ((i_pinf, 1.0), (i_pinf, -np.inf), (i_pinf, np.nan), (i_nan, 1.0), (i_nan, np.inf), (i_ninf, np.inf), (i_ninf, 0.0)):
        bad = y.copy()
        bad[row] = wrong
        _refused(bad, off, col, val, x)
    # a finite row next to them is still held to the bound, and a NaN there is still refused
    i_fin = int(np.nonzero((cls == 0) & (lens > 0))[0][0])
    bad = y.copy()
    bad[i_fin] = np.nan
    _refused(bad, off, col, val, x)
    bad = y.copy()
    bad[i_fin] = dtype(float(y[i_fin]) + 2 * REL_TOL[np.dtype(dtype)] * oracle.spmv_abs(off, col, val, x)[i_fin])
    _refused(bad, off, col, val, x)
    # all rows non-finite: nothing left for the bounds, and that is fine
    xn = np.full(200, np.nan, dtype)
    yn = oracle.spmv(off, col, val, xn)
    assert_spmv_close(yn.copy(), off, col, val, xn, "all NaN x")
    assert (yn[lens == 0] == 0).all() and np.isnan(yn[lens > 0]).all()


@DTYPES
def test_bucket_log_stays_valid_json(dtype, capsys):
    off, col, val, x, lens = _matrix(dtype)
    x = x.copy()
    x[::7] = np.nan
    x[3::11] = np.inf
    y = oracle.spmv(off, col, val, x)
    assert not np.isfinite(y).all()
    assert_spmv_close(y, off, col, val, x, "log")
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("parity buckets ")]
    assert lines
    for ln in lines:
        rec = json.loads(ln[len("parity buckets "):], parse_constant=lambda c: pytest.fail("not JSON: " + c))
        assert rec["rows"] == int(np.isfinite(y).sum())
    json.loads(json.dumps({"summary": PARITY_STATS}), parse_constant=lambda c: pytest.fail("not JSON: " + c))
