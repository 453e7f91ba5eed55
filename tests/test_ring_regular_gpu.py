"""K1r's regular phases (sparsemat_amd/csrc/spmv_ring2.hip, phase_rows<..., REG>): a ring phase whose rows are all L > 0 entries long
computes its row offsets instead of loading them -- same chunks, same lanes, same order of FMAs.  So y and inner_prod are the same
BITS with SMH_RING_REGULAR unset (the plan's table, SparseMatCRS.ring_regular) and =0 (no table: every phase loads its offsets), and
y is plain K1's (set_ring(0)) too.  (inner_prod is compared on / off only: K1 has no DOT form -- its inner_prod is the product
followed by a separate dot, whose sum has another order.)  Every test first asserts, through ring_regular() and ring_plan(), that
the phases it means to run are there."""
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


def window_crs(rng, n, lens, dtype=F):
    """Rows of lens[i] distinct columns from [i - 4096, i + 4096] within [0, n), ascending -- the window pattern."""
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    col = np.empty(int(off[-1]), np.uint32)
    for i in range(n):
        lo, hi = max(0, i - 4096), min(n - 1, i + 4096)
        col[off[i]:off[i + 1]] = np.sort(lo + rng.choice(hi - lo + 1, int(lens[i]), replace=False))
    val = rng.uniform(-1, 1, len(col)).astype(dtype)
    return off, col, val


def vectors(rng, n_rows, n_cols, dtype=F):
    return rng.uniform(-1, 1, n_cols).astype(dtype), rng.uniform(-1, 1, n_rows).astype(dtype)


def regular_model(off, phases):
    """The definition, restated: L for a ring phase (use_ring == 1) with L > 0 and off[r] == off[rb] + (r - rb) * L on [rb, re]."""
    off = off.astype(np.int64)
    out = np.zeros(len(phases), np.uint32)
    for p, ph in enumerate(phases):
        rb, re, use = int(ph[0]), int(ph[1]), int(ph[4])
        if use != 1 or re <= rb:
            continue
        L = off[rb + 1] - off[rb]
        if L > 0 and np.array_equal(off[rb:re + 1], off[rb] + np.arange(re - rb + 1) * L):
            out[p] = L
    return out


def plan_of(m, off):
    """(phases, reg_len) with the ring kernel asked for; the table is the model's."""
    m.set_ring(1)
    with env(SMH_RING_REGULAR=None, SMH_RING_COL12=None, SMH_RING_COL16=None):
        _, _, active, _, phases = m.ring_plan()
        reg = m.ring_regular()
    assert active and len(phases) > 1
    # the kernel that reads the table has the two ring bodies only: it runs for plans whose phases all gather from the ring
    assert (phases[:, 4] == 1).all() and reg.any()
    assert np.array_equal(reg, regular_model(off, phases))
    return phases, reg


def same_bits_on_and_off(m, x, lhs, form):
    """The product and inner_prod through the ring kernel with the table (unset) and without it (=0), and the product through K1."""
    m.set_ring(1)
    got = {}
    for v in (None, "0"):
        with env(SMH_RING_REGULAR=v, SMH_RING_COL12=None, SMH_RING_COL16=None):
            assert m.ring_column_form() == form  # (the REG body exists for the two narrow forms; the table changes no form)
            got[v] = (m.mvp(x, variant="vector"), m.inner_prod(lhs, x, variant="vector"))
    assert got[None][0].tobytes() == got["0"][0].tobytes()
    assert struct.pack("d", got[None][1]) == struct.pack("d", got["0"][1]), (got[None][1], got["0"][1])
    m.set_ring(0)
    with env(SMH_RING_REGULAR=None):
        y_k1 = m.mvp(x, variant="vector")
    m.set_ring(-1)
    assert y_k1.tobytes() == got[None][0].tobytes()
    return got[None][0]


def mixed_rows(seed, lens_of):
    """20 000 window rows of 32, except rows 5000 .. 5100 (at most three 64-row tiles) with lengths lens_of(rng, count)."""
    n = 20_000
    rng = np.random.default_rng(seed)
    lens = np.full(n, 32)
    lens[5000:5101] = lens_of(rng, 101)
    off, col, val = window_crs(rng, n, lens)
    return n, rng, off, col, val


@pytest.mark.parametrize("pattern", [synth.PATTERN_WINDOW, synth.PATTERN_BANDED], ids=["window", "stratified"])
def test_all_regular_col12(gpu, pattern):
    """20 000 rows x 32, f32 (no multiple of 64: the last phase ends in a clamped unit): every ring phase is regular with L = 32."""
    n = 20_000
    rng = np.random.default_rng(11)
    m = synth.crs_fixed(synth.SEED_MATRIX, pattern, n, 32, F)
    off = m.raw_parts()[0]
    phases, reg = plan_of(m, off)
    ring = phases[:, 4] == 1
    assert ring.any() and (reg[ring] == 32).all() and (reg[~ring] == 0).all()
    x, lhs = vectors(rng, n, n)
    same_bits_on_and_off(m, x, lhs, "col12")


def test_mixed_aligned_col12(gpu):
    """Lengths from {28, 32, 36} in rows 5000 .. 5100: chunks never straddle rows (AUTO keeps col12), the phases of those tiles are
    not regular, the others are."""
    n, rng, off, col, val = mixed_rows(12, lambda rng, k: rng.choice([28, 32, 36], k))
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    phases, reg = plan_of(m, off)
    ring = phases[:, 4] == 1
    assert (reg[ring] == 0).any() and (reg[ring] == 32).any()
    x, lhs = vectors(rng, n, n)
    same_bits_on_and_off(m, x, lhs, "col12")


def test_mixed_unaligned_col16(gpu):
    """Lengths from 20 .. 40 there: the regular phases behind them start inside a chunk and every row straddles chunks (col16)."""
    n, rng, off, col, val = mixed_rows(13, lambda rng, k: rng.integers(20, 41, k))
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    phases, reg = plan_of(m, off)
    ring = phases[:, 4] == 1
    assert (reg[ring] == 0).any() and (reg[ring] == 32).any()
    assert any(off[int(ph[0])] % 4 != 0 for ph, L in zip(phases, reg) if L)
    x, lhs = vectors(rng, n, n)
    same_bits_on_and_off(m, x, lhs, "col16")


@pytest.mark.parametrize("k", [31, 33])
def test_row_length_no_multiple_of_4(gpu, k):
    n = 20_000
    rng = np.random.default_rng(k)
    m = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, n, k, F)
    phases, reg = plan_of(m, m.raw_parts()[0])
    ring = phases[:, 4] == 1
    assert ring.any() and (reg[ring] == k).all()
    x, lhs = vectors(rng, n, n)
    same_bits_on_and_off(m, x, lhs, "col16")


def test_rows_longer_than_one_pass(gpu):
    """Rows of 48: AUTO keeps the ring; with 8 lanes per row (32 entry slots per pass) every row also takes the loop over its
    further passes."""
    n = 20_000
    rng = np.random.default_rng(48)
    m = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, n, 48, F)
    m.set_ring(-1)
    with env(SMH_RING_REGULAR=None, SMH_RING_COL12=None, SMH_RING_COL16=None):
        assert m.ring_plan()[2]  # (the ring is active by AUTO's own choice)
    phases, reg = plan_of(m, m.raw_parts()[0])
    ring = phases[:, 4] == 1
    assert ring.any() and (reg[ring] == 48).all()
    x, lhs = vectors(rng, n, n)
    with env(SMH_RING_COL12=None, SMH_RING_COL16=None):
        form = m.ring_column_form()
    assert form in ("col12", "col16")
    y = same_bits_on_and_off(m, x, lhs, form)
    m.set_vector_lanes(8)
    assert same_bits_on_and_off(m, x, lhs, form).shape == y.shape
    m.set_vector_lanes(0)


def test_unpadded_borrowed_arrays(gpu):
    """9 001 rows of 31 through from_device_parts: nnz % 4 == 3 -- regular phases together with the tail kernel."""
    n = 9_001
    rng = np.random.default_rng(6)
    off, col, val = window_crs(rng, n, np.full(n, 31))
    assert len(val) == 279_031 and len(val) % 4 == 3
    bufs = [synth.DeviceBuffer(a.nbytes) for a in (off, col, val)]
    for b, a in zip(bufs, (off, col, val)):
        b.upload(a)
    m = sm.SparseMatCRS.from_device_parts(n, n, len(val), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, F, keep=bufs)
    phases, reg = plan_of(m, off)
    ring = phases[:, 4] == 1
    assert ring.any() and (reg[ring] == 31).all()
    x, lhs = vectors(rng, n, n)
    y = same_bits_on_and_off(m, x, lhs, "col16")
    owned = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    plan_of(owned, off)
    assert same_bits_on_and_off(owned, x, lhs, "col16").tobytes() == y.tobytes()


def test_f64(gpu):
    """f64 rows of 32: regular, the 16-bit columns, the 1024-thread configuration."""
    n = 20_000
    rng = np.random.default_rng(7)
    m = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, n, 32, np.float64)
    phases, reg = plan_of(m, m.raw_parts()[0])
    ring = phases[:, 4] == 1
    assert ring.any() and (reg[ring] == 32).all()
    x, lhs = vectors(rng, n, n, np.float64)
    same_bits_on_and_off(m, x, lhs, "col16")


def test_empty_rows_are_not_regular(gpu):
    """8 192 empty rows, then window rows of 32: a phase of empty rows has L = 0 and reports 0."""
    n = 20_000
    rng = np.random.default_rng(8)
    lens = np.full(n, 32)
    lens[:8192] = 0
    off, col, val = window_crs(rng, n, lens)
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    phases, reg = plan_of(m, off)
    empty = np.array([off[int(ph[1])] == off[int(ph[0])] for ph in phases])
    ring = phases[:, 4] == 1
    assert empty.any() and (reg[empty] == 0).all() and (reg[ring & ~empty] == 32).all() and (ring & ~empty).any()
    x, lhs = vectors(rng, n, n)
    with env(SMH_RING_COL12=None, SMH_RING_COL16=None):
        form = m.ring_column_form()
    assert form in ("col12", "col16")
    same_bits_on_and_off(m, x, lhs, form)
