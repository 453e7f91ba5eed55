"""K1r's chunk records with 24-bit fixed-point values (sparsemat_amd/csrc/ring_val24.hpp; k_spmv_ring2's kRec16 form) against the
forms they replace, f32: the records change what the ring phases stream -- one 16-byte record per chunk instead of four floats and
four low column bytes -- never a value, so y and inner_prod are the same BITS with SMH_RING_VAL24 unset and =0, with the compact
column form off, through plain K1 and in the CPU model of the lane sums (oracle.spmv_lanes).  SparseMatCRS.ring_value_form() says
which form a handle resolved to; every test asserts it, so that no comparison runs the same kernel twice."""
import contextlib
import os
import struct

import numpy as np
import pytest

import oracle
import sparsemat_amd as sm
from sparsemat_amd import synth

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = [3_000, 50_000]
PATTERNS = [pytest.param(synth.PATTERN_WINDOW, id="window"), pytest.param(synth.PATTERN_BANDED, id="stratified")]
KNOBS = dict(SMH_RING_VAL24=None, SMH_RING_COL12=None, SMH_RING_COL16=None, SMH_RING_REGULAR=None)


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


def knobs(**kv):
    return env(**dict(KNOBS, **kv))


def fixed_point(rng, count, exponent=-23):
    """count values k * 2^exponent, k uniform in [-2^23, 2^23), the extremes and zero among them."""
    k = rng.integers(-2 ** 23, 2 ** 23, count)
    k[:3] = [-2 ** 23, 2 ** 23 - 1, 0]
    return np.ldexp(k.astype(np.float64), exponent).astype(F)


def gap_crs(rng, n, lens):
    """Rows of lens[i] ascending distinct columns with random gaps, inside a window of at most 8000 columns around the diagonal:
    one sliding window of the 16384-column ring, and four consecutive columns never further apart than the compact form holds."""
    lens = np.asarray(lens, np.int64)
    lmax = max(int(lens.max()), 1)
    g = max(1, min(8000 // lmax, (n - 1) // (lmax + 1), 250))
    gaps = rng.integers(1, g + 1, (n, lmax))
    rel = np.cumsum(gaps, axis=1) - gaps[:, :1]
    lo = np.clip(np.arange(n) - rel[:, -1] // 2, 0, n - 1 - rel[:, -1])
    cols = lo[:, None] + rel
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    col = cols[np.arange(lmax)[None, :] < lens[:, None]].astype(np.uint32)
    assert len(col) == off[-1] and col.max() < n
    return off, col


def vectors(rng, n_rows, n_cols):
    return rng.uniform(-1, 1, n_cols).astype(F), rng.uniform(-1, 1, n_rows).astype(F)


def product(m, x, lhs):
    return m.mvp(x, variant="vector"), struct.pack("d", m.inner_prod(lhs, x, variant="vector"))


def same_nan_aware(a, b):
    """Bit for bit, except that a NaN need only be a NaN: which payload a NaN operand leaves in an FMA differs between the CPU the
    model runs on and the GPU."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def model(m, off, col, val, x, borrowed=False):
    return oracle.spmv_lanes(off, col, val, x, m.resolved_variant()[1], tail_from=(len(val) & ~3) if borrowed else None)


def records_against_the_other_forms(m, x, lhs, exponent, column_knob=None):
    """With the knobs at their defaults (or SMH_RING_COL12 = column_knob) the handle streams records with this exponent; the product
    and inner_prod then have the bits of the same build without records.  Returns y."""
    m.set_ring(1)
    with knobs(SMH_RING_COL12=column_knob):
        assert m.ring_value_form() == ("val24", exponent) and m.ring_column_form() == "col12"
        got = product(m, x, lhs)
        assert m.ring_value_form() == ("val24", exponent)
    with knobs(SMH_RING_COL12=column_knob, SMH_RING_VAL24="0"):
        assert m.ring_value_form() == ("plain", None) and m.ring_column_form() == "col12"
        off24 = product(m, x, lhs)
    with knobs(SMH_RING_COL12=column_knob, SMH_RING_VAL24="1"):  # (1 is automatic: back to the records)
        assert m.ring_value_form() == ("val24", exponent)
        again = product(m, x, lhs)
    assert got[0].tobytes() == off24[0].tobytes() == again[0].tobytes() and got[1] == off24[1] == again[1]
    m.set_ring(-1)
    return got[0]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_generated_matrices_take_the_records_and_keep_every_bit(gpu, n, pattern):
    """The synthetic generators draw k * 2^-23 - 1 from 24 bits: adopted with E = -23; same bits with the knob at 0, with the compact
    column form off (16-bit columns and the value array), through K1, and in the CPU model."""
    rng = np.random.default_rng(n)
    m = synth.crs_fixed(synth.SEED_MATRIX, pattern, n, 32, F)
    off, col, val = m.raw_parts()
    x, lhs = vectors(rng, n, n)
    y = records_against_the_other_forms(m, x, lhs, -23)
    m.set_ring(1)
    with knobs(SMH_RING_COL12="0"):
        assert m.ring_value_form() == ("plain", None) and m.ring_column_form() == "col16"
        y16, d16 = product(m, x, lhs)
    with knobs():
        assert m.ring_value_form() == ("val24", -23)
        d24 = product(m, x, lhs)[1]
        m.set_ring(0)
        y_k1 = m.mvp(x, variant="vector")
        m.set_ring(-1)
        assert m.ring_value_form() == ("val24", -23)  # (AUTO's own choice too)
        assert m.mvp(x, variant="vector").tobytes() == y.tobytes()
    assert y16.tobytes() == y.tobytes() and d16 == d24 and y_k1.tobytes() == y.tobytes()
    assert model(m, off, col, val, x).tobytes() == y.tobytes()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,exponent", [("integers", 0), ("times4", -21)])
def test_other_exponents(gpu, kind, exponent, n):
    """Integers in [-8, 8] (E = 0: some value is odd) and the generator's values times 4 (E = -21)."""
    rng = np.random.default_rng(n + exponent)
    off, col, val = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, n, 32, F).raw_parts()
    val = rng.integers(-8, 9, len(val)).astype(F) if kind == "integers" else val * F(4)
    if kind == "integers":
        val[:2] = [1, -7]
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    x, lhs = vectors(rng, n, n)
    y = records_against_the_other_forms(m, x, lhs, exponent)
    assert model(m, off, col, val, x).tobytes() == y.tobytes()


BAD_VALUES = {"tenth": F(0.1), "minus-zero": F(-0.0), "nan": F(np.nan), "subnormal": np.array([5], np.uint32).view(F)[0]}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bad", list(BAD_VALUES))
def test_one_value_that_does_not_fit_refuses_the_matrix(gpu, bad, n):
    """One entry in the middle of the matrix replaced: the accessor reports the refusal, the compact column form stays, and y is the
    model's -- the path of a build without records."""
    rng = np.random.default_rng(n)
    off, col, val = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, n, 32, F).raw_parts()
    val[len(val) // 2 + 1] = BAD_VALUES[bad]
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    x, lhs = vectors(rng, n, n)
    m.set_ring(1)
    with knobs():
        assert m.ring_value_form() == ("refused", None) and m.ring_column_form() == "col12"
        y, d = product(m, x, lhs)
    with knobs(SMH_RING_VAL24="1"):  # (cannot be forced)
        assert m.ring_value_form() == ("refused", None)
    with knobs(SMH_RING_VAL24="0"):
        y0, d0 = product(m, x, lhs)
    want = model(m, off, col, val, x)
    assert same_nan_aware(y, want) and same_nan_aware(y, y0) and (d == d0 or bad == "nan")
    assert np.isnan(y).sum() == (1 if bad == "nan" else 0)


@pytest.mark.parametrize("n", SIZES)
def test_update_values_and_scale_test_the_new_values(gpu, n):
    """Eligible -> general floats -> eligible (another exponent) through update_values, then scale by 1/2 (still fixed-point, E - 1)
    and by 0.3 (not): the form goes and returns with the values, and every product is the model's of the values of the moment."""
    rng = np.random.default_rng(n)
    off, col, val = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_BANDED, n, 32, F).raw_parts()
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    x, lhs = vectors(rng, n, n)
    m.set_ring(1)
    general = rng.uniform(-1, 1, len(val)).astype(F)
    coarse = fixed_point(rng, len(val), -10)
    with knobs():
        steps = [(val, ("val24", -23)), (general, ("refused", None)), (coarse, ("val24", -10)), (general, ("refused", None)), (val, ("val24", -23))]
        for i, (values, form) in enumerate(steps):
            if i:
                m.update_values(values)
            assert m.ring_value_form() == form and m.ring_column_form() == "col12"
            assert m.mvp(x, variant="vector").tobytes() == model(m, off, col, values, x).tobytes(), form
        m.scale(0.5)
        assert m.ring_value_form() == ("val24", -24)
        assert m.mvp(x, variant="vector").tobytes() == model(m, off, col, val * F(0.5), x).tobytes()
        m.scale(0.3)
        assert m.ring_value_form() == ("refused", None)
        assert m.mvp(x, variant="vector").tobytes() == model(m, off, col, m.raw_parts()[2], x).tobytes()


@pytest.mark.parametrize("k", [31, 33])
def test_rows_that_straddle_chunks_keep_col16_and_build_no_records(gpu, k):
    """31 / 33 entries per row: the compact column form escapes everywhere, AUTO keeps the 16-bit columns, so there are no records
    (and the values are never tested).  Forced (SMH_RING_COL12=1) the records carry side-table indices in their fourth dword: same
    bits as the 16-bit columns."""
    n = 20_000
    rng = np.random.default_rng(k)
    m = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, n, k, F)
    off, col, val = m.raw_parts()
    x, lhs = vectors(rng, n, n)
    m.set_ring(1)
    with knobs():
        assert m.ring_column_form() == "col16" and m.ring_value_form() == ("plain", None)
        y16, d16 = product(m, x, lhs)
    y = records_against_the_other_forms(m, x, lhs, -23, column_knob="1")
    m.set_ring(1)
    with knobs(SMH_RING_COL12="1"):
        d = product(m, x, lhs)[1]
    with knobs():
        assert m.ring_column_form() == "col16" and m.ring_value_form() == ("plain", None)
    assert y.tobytes() == y16.tobytes() and d == d16
    assert model(m, off, col, val, x).tobytes() == y.tobytes()


def test_a_phase_that_begins_inside_a_chunk(gpu):
    """101 rows of 31, then rows of 32: every later phase starts at an entry that is 3 mod 4 -- its first chunk belongs to the phase
    before it -- and every row straddles chunks, so the compact form is forced."""
    n = 20_000
    rng = np.random.default_rng(31)
    lens = np.full(n, 32)
    lens[:101] = 31
    off, col = gap_crs(rng, n, lens)
    val = fixed_point(rng, len(col))
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    m.set_ring(1)
    with knobs(SMH_RING_COL12="1"):
        phases, reg = m.ring_plan()[4], m.ring_regular()
    assert any(L and off[int(ph[0])] % 4 == 3 for ph, L in zip(phases, reg))
    x, lhs = vectors(rng, n, n)
    y = records_against_the_other_forms(m, x, lhs, -23, column_knob="1")
    assert model(m, off, col, val, x).tobytes() == y.tobytes()


def test_borrowed_unpadded_arrays_with_the_tail_kernel(gpu):
    """Rows of 32 and a last row of 35 through from_device_parts: nnz % 4 == 3 -- the records end at the last whole chunk, the tail
    kernel adds the rest from the value array."""
    n = 9_000
    rng = np.random.default_rng(35)
    lens = np.full(n, 32)
    lens[-1] = 35
    off, col = gap_crs(rng, n, lens)
    val = fixed_point(rng, len(col))
    assert len(val) % 4 == 3
    bufs = [synth.DeviceBuffer(a.nbytes) for a in (off, col, val)]
    for b, a in zip(bufs, (off, col, val)):
        b.upload(a)
    m = sm.SparseMatCRS.from_device_parts(n, n, len(val), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, F, keep=bufs)
    x, lhs = vectors(rng, n, n)
    y = records_against_the_other_forms(m, x, lhs, -23)
    assert model(m, off, col, val, x, borrowed=True).tobytes() == y.tobytes()


def test_long_rows_and_empty_rows(gpu):
    """Rows of 100 (with 8 lanes per row the loop over a row's further passes decodes records too) between rows of 32, runs of empty
    rows and single ones: phases that load their offsets and phases that compute them, in one launch."""
    n = 12_000
    rng = np.random.default_rng(100)
    lens = np.full(n, 32)
    lens[4000:4200] = 100
    lens[7000:7300] = 0
    lens[::97] = 0
    off, col = gap_crs(rng, n, lens)
    val = fixed_point(rng, len(col))
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    m.set_ring(1)
    with knobs():
        reg = m.ring_regular()
    assert (reg == 0).any() and (reg == 32).any()
    x, lhs = vectors(rng, n, n)
    for lanes in (0, 8, 4):
        m.set_vector_lanes(lanes)
        y = records_against_the_other_forms(m, x, lhs, -23)
        assert model(m, off, col, val, x).tobytes() == y.tobytes(), lanes
    m.set_vector_lanes(0)


@pytest.mark.parametrize("n", SIZES)
def test_four_block_partitioned_product(gpu, n):
    """SparseMatPar with four blocks on one device, overlap on and off: boundary rows go through K1 from the value array, interior
    rows through the records -- the same y as without records and as the whole matrix's product."""
    rng = np.random.default_rng(n)
    off, col, val = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, n, 32, F).raw_parts()
    x = rng.uniform(-1, 1, n).astype(F)
    par = sm.SparseMatParLocal.with_sub_matrices(4, n, n, off, col, val, device_ids=[0, 0, 0, 0])
    ys = {}
    for overlap in (True, False):
        par.set_overlap(overlap)
        for v in (None, "0"):
            with knobs(SMH_RING_VAL24=v):
                ys[(overlap, v)] = par.mvp(x, variant="vector").tobytes()
    par.set_overlap(True)
    whole = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    with knobs():
        y = whole.mvp(x, variant="vector")
        assert whole.ring_value_form() == ("val24", -23)
    assert set(ys.values()) == {y.tobytes()}
