"""K1r's all-regular form (sparsemat_amd/csrc/spmv_ring2_allreg.hip, k_spmv_ring2_allreg): an f32 plan on the 16384-slot ring whose
phases are ALL regular runs the regular body alone, in workgroups of 768 threads -- 12 waves, so a wave's units are 12 units apart
(lanes 8: 192 rows) where the 512-thread kernels step by 8 (128 rows).  Which wave takes a row changes, what is done to the row does
not: y is the same BITS with SMH_RING_ALLREG unset and =0 (the REGK kernel), with SMH_RING_REGULAR=0 (every phase loads its offsets),
through plain K1 (set_ring(0)) and in oracle.spmv_lanes.  The form each side took is asserted through ring_launch_form() before and
after its products, and the phase sizes a case is about through ring_plan().  SMH_RING_BLOCKS_PER_CU=1 (read when the plan is
built) cuts a matrix into as many row ranges as the device has CUs, which gives long phases on small matrices."""
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
KNOBS = ("SMH_RING_ALLREG", "SMH_RING_REGULAR", "SMH_RING_COL12", "SMH_RING_COL16", "SMH_RING_VAL24", "SMH_RING_WIDE", "SMH_RING_BANDS")


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


@pytest.fixture
def one_range_per_cu(gpu):
    """Plans of one row range per CU, every other ring knob unset; yields that number of row ranges (B)."""
    with env(SMH_RING_BLOCKS_PER_CU="1", **{k: None for k in KNOBS}):
        probe = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, 4096, 32, F)
        probe.set_ring(1)
        yield probe.ring_plan()[0]


def shape_rows(name, B):
    """(n_rows, the phase sizes the plan must hold) of a matrix cut into B row ranges of whole 64-row tiles (the last one ends with
    the matrix), for window rows, whose phases are whole row ranges."""
    return {
        "5": (256 * (B - 1) + 5, {256, 5}),            # a phase of fewer than 16 rows: one unit, most of its rows clamped away
        "100": (256 * (B - 1) + 100, {256, 100}),      # 7 units: waves 7 .. 11 have none
        "192": (192 * B, {192}),                       # one unit per wave, no second trip
        "193": (256 * (B - 1) + 193, {256, 193}),      # ... and one row of a second unit for wave 0
        "383_384": (384 * B - 1, {384, 383}),          # two strides, the last unit one row short / full
        "385": (448 * (B - 1) + 385, {448, 385}),      # two strides and a row
        "640": (640 * B, {640}),                       # several strides
    }[name]


SHAPES = ["5", "100", "192", "193", "383_384", "385", "640"]


def phase_sizes(m):
    _, _, active, _, phases = m.ring_plan()
    assert active and (phases[:, 4] == 1).all()
    return set(int(v) for v in phases[:, 1] - phases[:, 0])


def product(m, x, form, **knobs):
    """y of the ring kernel under `knobs`, with the form it says it launches -- before and after -- equal to `form`."""
    with env(**knobs):
        before = m.ring_launch_form()
        y = m.mvp(x, variant="vector")
        assert m.ring_launch_form() == before
    assert before[0] == form, (before, form, knobs)
    assert before[1:] == ((768, 2) if form == 2 else (512, 2)), before
    return y


def four_ways(m, off, col, val, x, form=2, tail_from=None):
    """The product through the form the matrix takes by itself (`form`), the REGK kernel, the kernel without the table, K1 and the
    model of the lanes' sums: one y, bit for bit.  tail_from (borrowed arrays that end inside a chunk, nnz & ~3): every ring kernel
    leaves the entries from there on to the tail kernel, which adds them to their rows' stored sums, where K1 gives them to the
    lanes that own them (tests/test_spmv_order_gpu.py) -- the model has both orders, and K1 is compared on the rows before them."""
    m.set_ring(1)
    lanes = m.resolved_variant()[1]
    y = product(m, x, form)
    assert product(m, x, 1, SMH_RING_ALLREG="0").tobytes() == y.tobytes()
    assert product(m, x, 0, SMH_RING_REGULAR="0").tobytes() == y.tobytes()
    assert product(m, x, form, SMH_RING_ALLREG="auto").tobytes() == y.tobytes()
    m.set_ring(0)
    assert m.ring_launch_form() == (-1, 0, 0)
    y_k1 = m.mvp(x, variant="vector")
    m.set_ring(1)
    whole = len(y) if tail_from is None else int(np.searchsorted(off, tail_from, side="right")) - 1  # rows without a tail entry
    assert y_k1[:whole].tobytes() == y[:whole].tobytes() and whole >= len(y) - 1
    assert y_k1.tobytes() == oracle.spmv_lanes(off, col, val, x, lanes).tobytes()
    assert oracle.spmv_lanes(off, col, val, x, lanes, tail_from=tail_from).tobytes() == y.tobytes()
    return y, lanes


def window(n, k):
    """n window rows of k entries from the project's generator, as a handle and on the host."""
    m = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, n, k, F)
    return (m,) + m.raw_parts()


@pytest.mark.parametrize("values", ["records", "plain"])
@pytest.mark.parametrize("shape", SHAPES)
def test_window_rows_of_32(one_range_per_cu, shape, values):
    """The headline's instantiation (lanes 8) over phases of every size at which the 12-wave stride could go wrong.  "records": the
    generator's values, 24-bit fixed point; "plain": values that are no multiples of one power of two -- col12 beside the value
    array.  Both take the form."""
    n, want = shape_rows(shape, one_range_per_cu)
    m, off, col, val = window(n, 32)
    if values == "plain":
        val = np.random.default_rng(1).uniform(-1, 1, len(val)).astype(F)
        m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    m.set_ring(1)
    assert want <= phase_sizes(m), (want, phase_sizes(m))
    assert m.ring_column_form() == "col12" and m.ring_value_form()[0] == ("val24" if values == "records" else "refused")
    x = np.random.default_rng(2).uniform(-1, 1, n).astype(F)
    _, lanes = four_ways(m, off, col, val, x)
    assert lanes == 8


@pytest.mark.parametrize("k", [31, 33])
def test_rows_of_31_and_33(one_range_per_cu, k):
    """Regular with L no multiple of 4: the 16-bit columns, rows that begin inside a chunk (three in four), and -- the generator's
    arrays are borrowed and end inside a chunk -- the tail kernel behind the form's launch.  An owned (padded) copy, which has
    no tail, gives the same y on the rows before the last.  (A PHASE of an all-regular plan cannot begin inside a chunk: phases begin at multiples of 64 rows and every phase before
    holds 64 k rows of one length, so its first entry is a multiple of 64.)"""
    n, want = shape_rows("193", one_range_per_cu)
    m, off, col, val = window(n, k)
    assert len(val) % 4 != 0
    m.set_ring(1)
    assert want <= phase_sizes(m)
    assert m.ring_column_form() == "col16"
    assert all(off[int(rb)] % 64 == 0 for rb in m.ring_plan()[4][:, 0]) and (off[:-1] % 4 != 0).sum() > n // 2
    x = np.random.default_rng(k).uniform(-1, 1, n).astype(F)
    y, _ = four_ways(m, off, col, val, x, tail_from=len(val) & ~3)
    owned = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    assert four_ways(owned, off, col, val, x)[0][:-1].tobytes() == y[:-1].tobytes()


def window_host(n, k, seed):
    """... built on the host (the generator draws at most 64 columns per row): row i holds k ascending columns from a window of 8000
    behind max(0, min(i - 4096, n - 8000)), gaps of 1 .. 79; values k * 2^-23, 24-bit integers k, like the generator's."""
    rng = np.random.default_rng(seed)
    assert n > 8000 and 79 * k < 8000
    start = np.clip(np.arange(n) - 4096, 0, n - 8000)
    col = (start[:, None] + rng.integers(1, 80, (n, k)).cumsum(axis=1)).astype(np.uint32).ravel()
    val = (rng.integers(-2**23, 2**23, n * k) * 2.0**-23).astype(F)
    off = (np.arange(n + 1, dtype=np.uint64) * k).astype(np.uint32)
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val), off, col, val


@pytest.mark.parametrize("k", [48, 100])
def test_rows_of_several_passes(one_range_per_cu, k):
    """Rows of 48 (lanes 16: one pass; forced to 8: two) and of 100 (lanes 32: 128 slots a pass; forced to 8: four passes)."""
    n, want = shape_rows("385", one_range_per_cu)
    m, off, col, val = window(n, k) if k <= 64 else window_host(n, k, k)
    m.set_ring(1)
    assert want <= phase_sizes(m)
    x = np.random.default_rng(k).uniform(-1, 1, n).astype(F)
    _, lanes = four_ways(m, off, col, val, x)
    assert lanes == (16 if k == 48 else 32)
    m.set_vector_lanes(8)
    assert four_ways(m, off, col, val, x)[1] == 8
    m.set_vector_lanes(0)


@pytest.mark.parametrize("shape", ["383_384", "385"])
def test_rows_of_16_at_lanes_4(one_range_per_cu, shape):
    """AUTO's 4 lanes for rows of 16: a unit is 32 rows, the stride 384."""
    n, want = shape_rows(shape, one_range_per_cu)
    m, off, col, val = window(n, 16)
    m.set_ring(1)
    assert want <= phase_sizes(m)
    x = np.random.default_rng(16).uniform(-1, 1, n).astype(F)
    assert four_ways(m, off, col, val, x)[1] == 4


@pytest.mark.parametrize("what", ["one row one entry shorter", "one empty row"])
def test_not_all_regular(one_range_per_cu, what):
    """One row of another length: its phase is not regular, the plan keeps the REGK kernel (form 1) whatever the knob says."""
    n, want = shape_rows("193", one_range_per_cu)
    _, off, col, val = window(n, 32)
    row = 1000
    keep = np.ones(len(val), bool)
    keep[off[row] + (31 if what.startswith("one row one") else 0):off[row + 1]] = False
    lens = np.diff(off.astype(np.int64))
    lens[row] = 31 if what.startswith("one row one") else 0
    off2 = np.concatenate(([0], np.cumsum(lens))).astype(np.uint32)
    col2, val2 = col[keep], val[keep]
    m = sm.SparseMatCRS.from_raw_parts(n, n, off2, col2, val2)
    m.set_ring(1)
    assert want <= phase_sizes(m)
    reg = m.ring_regular()
    assert (reg == 0).sum() == 1 and (reg == 32).sum() == len(reg) - 1
    x = np.random.default_rng(3).uniform(-1, 1, n).astype(F)
    lanes = m.resolved_variant()[1]
    y = product(m, x, 1)
    assert product(m, x, 1, SMH_RING_ALLREG="0").tobytes() == y.tobytes()
    assert product(m, x, 0, SMH_RING_REGULAR="0").tobytes() == y.tobytes()
    assert oracle.spmv_lanes(off2, col2, val2, x, lanes).tobytes() == y.tobytes()


def test_inner_prod_keeps_its_kernel(one_range_per_cu):
    """inner_prod's sum goes with the 8 waves of the 512-thread kernels: the same bits with the knob unset and at 0, and what a
    plain product would launch is the all-regular form before and after."""
    n, _ = shape_rows("385", one_range_per_cu)
    m, off, col, val = window(n, 32)
    m.set_ring(1)
    rng = np.random.default_rng(4)
    x, lhs = rng.uniform(-1, 1, n).astype(F), rng.uniform(-1, 1, n).astype(F)
    got = {}
    for knob in (None, "0"):
        with env(SMH_RING_ALLREG=knob):
            before = m.ring_launch_form()
            got[knob] = m.inner_prod(lhs, x, variant="vector")
            assert m.ring_launch_form() == before == ((2, 768, 2) if knob is None else (1, 512, 2))
    assert struct.pack("d", got[None]) == struct.pack("d", got["0"]), got
    y = product(m, x, 2)
    assert abs(got[None] - float(np.dot(lhs.astype(np.float64), y.astype(np.float64)))) <= 1e-3 * np.abs(lhs * y).sum()


def test_partition_of_four_blocks(gpu):
    """Four blocks of an all-regular matrix on one device: the overlapped product (interior row ranges beside the exchange,
    boundary rows apart) and the plain one are the same bits, with the knob unset and at 0, and the model's."""
    n = 100_000
    with env(**{k: None for k in KNOBS}):
        _, off, col, val = window(n, 32)
        x = np.random.default_rng(5).uniform(-1, 1, n).astype(F)
        want = oracle.spmv_lanes(off, col, val, x, 8)
        m = sm.SparseMatParLocal.with_sub_matrices(4, n, n, off, col, val, device_ids=[0] * 4)
        assert all(m.interior(b, "vector")[1] > m.interior(b, "vector")[0] for b in range(4))
        for knob in (None, "0"):
            for overlap in (True, False):
                with env(SMH_RING_ALLREG=knob):
                    m.set_overlap(overlap)
                    xv, yv = m.vec(host=x), m.vec()
                    m.mvp_dev(xv, yv, variant="vector")
                    m.synchronize()
                    assert yv.download().tobytes() == want.tobytes(), (knob, overlap)
        # (a block of these rows by itself: the form the partition's blocks take)
        b0 = sm.SparseMatCRS.from_raw_parts(25_000, n, off[:25_001], col[:off[25_000]], val[:off[25_000]])
        b0.set_ring(1)
        assert b0.ring_launch_form() == (2, 768, 2)


def test_two_workgroups_of_768_threads_per_cu(gpu):
    """The premise: the runtime holds TWO 768-thread workgroups of the headline's instantiation (f32, lanes 8, chunk records,
    66 KiB of LDS each) on a CU -- 24 wavefronts.  One per CU would be 12 wavefronts, fewer than the 16 of the REGK kernel."""
    with env(**{k: None for k in KNOBS}):
        m = synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, 50_000, 32, F)
        assert m.resolved_variant() == ("vector", 8) and m.ring_value_form()[0] == "val24"
        form = m.ring_launch_form()
    assert form[:2] == (2, 768), form
    assert form[2] == 2, ("the runtime answers %d resident 768-thread workgroup(s) per CU for the all-regular kernel: the premise of "
                          "the form -- two of them, 24 wavefronts per CU -- is false on this stack" % form[2])


def test_update_values_and_scale(one_range_per_cu):
    """New values drop the chunk records; they are rebuilt, the form stays, y is K1's and the model's."""
    n, _ = shape_rows("193", one_range_per_cu)
    m, off, col, val = window(n, 32)
    m.set_ring(1)
    x = np.random.default_rng(6).uniform(-1, 1, n).astype(F)
    four_ways(m, off, col, val, x)
    m.scale(0.5)
    val = (val * F(0.5)).astype(F)
    assert m.ring_value_form()[0] == "val24"
    four_ways(m, off, col, val, x)
    val = np.ascontiguousarray(val[::-1])
    m.update_values(val)
    assert m.ring_value_form()[0] == "val24"
    four_ways(m, off, col, val, x)
    val = np.random.default_rng(7).uniform(-1, 1, len(val)).astype(F)  # ... and values the records cannot hold: col12 beside the values
    m.update_values(val)
    assert m.ring_value_form()[0] == "refused"
    four_ways(m, off, col, val, x)
