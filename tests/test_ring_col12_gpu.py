"""K1r's compact column form (12 bits per column: sparsemat_amd/csrc/ring_col12.hpp) against the 16-bit columns, f32: the form
changes what the ring phases stream, never a slot -- so y and inner_prod are the same BITS with SMH_RING_COL12=1 and =0 -- and
which form a handle resolves to (SparseMatCRS.ring_column_form)."""
import contextlib
import os
import struct

import numpy as np
import pytest

import sparsemat_amd as sm
from sparsemat_amd import synth

pytestmark = pytest.mark.gpu
F = np.float32


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def window_crs(rng, n, lens, descending=False):
    """Rows of lens[i] distinct columns from [i - 4096, i + 4096] within [0, n), ascending (or descending) -- the window pattern."""
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    col = np.empty(int(off[-1]), np.uint32)
    for i in range(n):
        lo, hi = max(0, i - 4096), min(n - 1, i + 4096)
        c = np.sort(lo + rng.choice(hi - lo + 1, int(lens[i]), replace=False))
        col[off[i]:off[i + 1]] = c[::-1] if descending else c
    val = rng.uniform(-1, 1, len(col)).astype(F)
    return off, col, val


def same_bits_in_both_forms(m, x, lhs, expect_form_off=("col16",)):
    """The product and inner_prod through the ring kernel with the compact form forced and with it switched off."""
    m.set_ring(1)
    got = {}
    for v in ("1", "0"):
        with env(SMH_RING_COL12=v, SMH_RING_COL16=None):
            y = m.mvp(x, variant="vector")
            got[v] = (y, m.ring_column_form(), m.inner_prod(lhs, x, variant="vector"))
    assert got["1"][1] == "col12" and got["0"][1] in expect_form_off, (got["1"][1], got["0"][1])
    assert got["1"][0].tobytes() == got["0"][0].tobytes()
    assert struct.pack("d", got["1"][2]) == struct.pack("d", got["0"][2]), (got["1"][2], got["0"][2])
    m.set_ring(-1)
    return got["1"][0]


def vectors(rng, n_rows, n_cols):
    return rng.uniform(-1, 1, n_cols).astype(F), rng.uniform(-1, 1, n_rows).astype(F)


@pytest.mark.parametrize("pattern", [synth.PATTERN_WINDOW, synth.PATTERN_BANDED], ids=["window", "stratified"])
def test_generated_patterns_take_the_compact_form_by_themselves(gpu, pattern):
    """20 000 rows x 32 (several row ranges and phases): AUTO resolves to the compact form; an explicit SMH_RING_COL16 keeps its
    meaning and switches that choice off; set_ring(0) then set_ring(-1) changes neither the form nor the result."""
    n = 20_000
    rng = np.random.default_rng(1)
    m = synth.crs_fixed(synth.SEED_MATRIX, pattern, n, 32, F)
    x, lhs = vectors(rng, n, n)
    with env(SMH_RING_COL12=None, SMH_RING_COL16=None):
        y_auto = m.mvp(x, variant="vector")
        assert m.ring_plan()[2] and m.ring_column_form() == "col12"
    y = same_bits_in_both_forms(m, x, lhs)
    assert y.tobytes() == y_auto.tobytes()
    with env(SMH_RING_COL12=None, SMH_RING_COL16="1"):
        assert m.ring_column_form() == "col16" and m.mvp(x, variant="vector").tobytes() == y.tobytes()
    with env(SMH_RING_COL12=None, SMH_RING_COL16="0"):
        assert m.ring_column_form() == "u32" and m.mvp(x, variant="vector").tobytes() == y.tobytes()
    with env(SMH_RING_COL12=None, SMH_RING_COL16=None):
        assert m.ring_column_form() == "col12"
        m.set_ring(0)
        y_k1 = m.mvp(x, variant="vector")
        m.set_ring(-1)
        assert m.ring_column_form() == "col12" and m.mvp(x, variant="vector").tobytes() == y.tobytes()
        assert y_k1.tobytes() == y.tobytes()  # (K1 is K1r bit for bit)
        # sort_rows (a no-op on these rows) drops the form with the storage order; it comes back the same
        m.sort_rows()
        assert m.ring_column_form() == "col12" and m.mvp(x, variant="vector").tobytes() == y.tobytes()


@pytest.mark.parametrize("k", [31, 33])
def test_rows_that_straddle_chunks_escape_on_every_row(gpu, k):
    """31 / 33 entries per row: most chunks hold the end of one row and the start of the next, which the code cannot hold --
    AUTO keeps the 16-bit columns, the forced compact form takes the escape branch everywhere."""
    n = 20_000
    rng = np.random.default_rng(k)
    m = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, n, k, F)
    x, lhs = vectors(rng, n, n)
    with env(SMH_RING_COL12=None, SMH_RING_COL16=None):
        assert m.ring_column_form() == "col16"
        y_auto = m.mvp(x, variant="vector")
    assert same_bits_in_both_forms(m, x, lhs).tobytes() == y_auto.tobytes()
    with env(SMH_RING_COL12=None, SMH_RING_COL16=None):
        assert m.ring_column_form() == "col16"  # (having been forced once does not change what AUTO takes)


def test_unpadded_arrays_with_a_partial_last_chunk(gpu):
    """Borrowed arrays with nnz % 4 != 0: the streaming kernel stops at the last whole chunk, the tail kernel adds the rest."""
    n = 9_000
    rng = np.random.default_rng(3)
    lens = rng.integers(20, 40, n)
    lens[-1] += 3 - int(lens.sum()) % 4  # nnz % 4 == 3
    off, col, val = window_crs(rng, n, lens)
    assert len(val) % 4 == 3
    bufs = [synth.DeviceBuffer(a.nbytes) for a in (off, col, val)]
    for b, a in zip(bufs, (off, col, val)):
        b.upload(a)
    m = sm.SparseMatCRS.from_device_parts(n, n, len(val), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, F, keep=bufs)
    x, lhs = vectors(rng, n, n)
    y = same_bits_in_both_forms(m, x, lhs)
    owned = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    assert same_bits_in_both_forms(owned, x, lhs).tobytes() == y.tobytes()


def test_empty_rows_and_one_long_row(gpu):
    """Rows of 0..40 entries, runs of empty rows and one row of 300: the loop over the passes of a long row decodes too."""
    n = 12_000
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 41, n)
    lens[3000:3200] = 0
    lens[::97] = 0
    lens[5000] = 300
    off, col, val = window_crs(rng, n, lens)
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    x, lhs = vectors(rng, n, n)
    for lanes in (0, 4, 8):
        m.set_vector_lanes(lanes)
        same_bits_in_both_forms(m, x, lhs)


def test_escape_by_span_and_by_order(gpu):
    """Four consecutive columns that span more than 17 strata of 256, and columns stored descending: both leave the code
    through the side table."""
    n = 12_000
    rng = np.random.default_rng(5)
    lens = np.full(n, 32)
    off, col, val = window_crs(rng, n, lens)
    for r in range(4200, 7800, 3):  # the first chunk of these rows: i - 4000, i - 100, i + 3000, i + 4090 (sorted, 8090 columns wide)
        c = col[off[r]:off[r + 1]].copy()
        c[:4] = [r - 4000, r - 100, r + 3000, r + 4090]
        c[4:] = r + 4091 + np.arange(28)  # (still ascending and distinct; inside [0, n))
        col[off[r]:off[r + 1]] = c
    assert col.max() < n
    x, lhs = vectors(rng, n, n)
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    y = same_bits_in_both_forms(m, x, lhs)
    with env(SMH_RING_COL12=None, SMH_RING_COL16=None):
        assert m.ring_column_form() == "col16"  # 1200 escaped chunks in 96 000: more than one in 1024
    # one such row alone stays under the limit: AUTO takes the compact form with its escape
    off1, col1, val1 = window_crs(rng, n, lens)
    r = 6000
    col1[off1[r]:off1[r] + 4] = [r - 4000, r - 100, r + 3000, r + 4090]
    col1[off1[r] + 4:off1[r + 1]] = r + 4091 + np.arange(28)
    m1 = sm.SparseMatCRS.from_raw_parts(n, n, off1, col1, val1)
    with env(SMH_RING_COL12=None, SMH_RING_COL16=None):
        assert m1.ring_column_form() == "col12"
        y1 = m1.mvp(x, variant="vector")
    assert same_bits_in_both_forms(m1, x, lhs).tobytes() == y1.tobytes()
    # descending inside the window
    offd, cold, vald = window_crs(rng, n, lens, descending=True)
    md = sm.SparseMatCRS.from_raw_parts(n, n, offd, cold, vald)
    same_bits_in_both_forms(md, x, lhs)
    with env(SMH_RING_COL12=None, SMH_RING_COL16=None):
        assert md.ring_column_form() == "col16"
    assert y is not None


def test_two_block_partitioned_product(gpu):
    """SparseMatPar with two blocks on one device: the blocks' boundary and interior rows are launched over parts of the plan."""
    n = 40_000
    rng = np.random.default_rng(6)
    off, col, val = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, n, 32, F).raw_parts()
    x = rng.uniform(-1, 1, n).astype(F)
    par = sm.SparseMatParLocal.with_sub_matrices(2, n, n, off, col, val, device_ids=[0, 0])
    ys = {}
    for v in ("1", "0"):
        with env(SMH_RING_COL12=v, SMH_RING_COL16=None):
            ys[v] = par.mvp(x, variant="vector")
    assert ys["1"].tobytes() == ys["0"].tobytes()
    whole = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    with env(SMH_RING_COL12="1", SMH_RING_COL16=None):
        assert whole.mvp(x, variant="vector").tobytes() == ys["1"].tobytes()
