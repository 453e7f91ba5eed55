"""The cases of the inner_prod bit tests, shared by tests/test_inner_prod_model.py (CPU: the models against exact sums, and that each
case's data tells every wrong variant of its route apart) and tests/test_inner_prod_bits_gpu.py (the device against the models).
Nothing here touches the device."""
import functools

import numpy as np

import kernel_forms as kf
import oracle
from util import random_crs

F32, F64 = np.float32, np.float64
DTYPES = (F32, F64)
# row ranges ensure_ring_plan cuts a matrix into: 6 per compute unit, 256 of them on an MI355X (the wide ring: half as many).  The
# CPU tests plan with these; the device tests take the handle's own number and hold the handle's plan to the model's.
RING_BLOCKS, RING_BLOCKS_WIDE = 1536, 768


def lhs_vector(n, dtype, seed, last_rows=None):
    """uniform in (-1, 1) with some -0.0 and +0.0 among the entries; last_rows: +0 everywhere but on that many rows at the end (so that
    the share of a matrix's last entries is not lost in the sum of all the others)"""
    lhs = np.random.default_rng(seed).uniform(-1, 1, n).astype(dtype)
    lhs[3::53] = -0.0
    lhs[7::101] = 0.0
    if last_rows is not None:
        lhs[:max(0, n - last_rows)] = 0.0
    return lhs


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.uint32)
    np.cumsum(np.asarray(lens, np.int64), out=off[1:])
    return off


def near_diagonal(lens, n_cols, reach, dtype, seed, values=None):
    """(off, col, val): row i holds lens[i] entries within `reach` columns of i * n_cols / n_rows, in draw order (duplicates possible)"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    off = _offsets(lens)
    centre = (np.repeat(np.arange(n), lens) * n_cols) // max(n, 1)
    col = np.clip(centre + rng.integers(-reach, reach + 1, len(centre)), 0, n_cols - 1).astype(np.uint32)
    if values is None:
        val = rng.uniform(-1, 1, len(col)).astype(dtype)
    else:
        val = rng.choice(np.asarray(values, dtype), len(col))
    return off, col, val


# ---- K1r -------------------------------------------------------------------------------------------------------------------------
class RingCase:
    """build(dtype) -> (n_cols, off, col, val, x); widths: (lanes, chunks per lane; 0 = automatic) the handle is set to; borrowed:
    device arrays of exactly nnz entries; entries / bands / form: what the handle's getters must report (form None: not asserted);
    env: held through the case; envs: further settings under which the SAME bits must come out (regular phases on and off);
    planned: the single-window plan can be restated on the CPU (ipm.ring_plan_rows); tells: the wrong variants this case's data
    must tell apart (asserted on the CPU for the planned cases, in the device test for the others); seed, last_rows: of its lhs
    (lhs_vector) -- a seed is one at which the case's data does tell them all, in both value types: the result is ONE number, and
    an order that moves the last bit of a few partial sums moves the last bit of their sum only now and then"""

    def __init__(self, build, widths, tells, borrowed=False, entries=16384, bands=1, form=None, env=None, envs=({},), dtypes=DTYPES,
                 planned=True, force=True, seed=1, last_rows=None):
        self.build, self.widths, self.tells, self.borrowed, self.entries, self.bands = build, widths, tells, borrowed, entries, bands
        self.form, self.env, self.envs, self.dtypes, self.planned, self.force = form, env or kf.NO_RING_ENV, envs, dtypes, planned, force
        self.seed, self.last_rows = seed, last_rows

    def lhs(self, n_rows, dtype):
        return lhs_vector(n_rows, dtype, self.seed, self.last_rows)

    @property
    def n_blocks(self):
        return RING_BLOCKS_WIDE if self.entries == 32768 else RING_BLOCKS


def ragged_with(mod):
    def build(dtype):
        n_cols, off, col, val = kf.ragged(dtype, mod)
        return n_cols, off, col, val, kf.vector_x(n_cols, dtype)
    return build


def ragged_tail_over_two_rows(dtype):
    """the ragged matrix with nnz mod 4 == 2 and one more row of one entry: as borrowed arrays the last three entries -- two of row
    4100, the one of row 4101 -- go to the tail kernel"""
    n_cols, off, col, val = kf.ragged(dtype, 2)
    off = np.concatenate([off, [off[-1] + 1]]).astype(np.uint32)
    col = np.concatenate([col, [17]]).astype(np.uint32)
    val = np.concatenate([val, [0.625]]).astype(dtype)
    assert int(off[-1]) % 4 == 3 and int(off[-3]) < (int(off[-1]) & ~3) < int(off[-2])
    return n_cols, off, col, val, kf.vector_x(n_cols, dtype)


def config(name):
    return lambda dtype: kf.config_matrix(name, dtype)


@functools.lru_cache(maxsize=None)
def _short_rows(dtname):
    dtype = np.dtype(dtname).type
    n = 100_003  # 1563 tiles of 64 rows: two per row range, so a phase holds two units of a wave and more
    off, col, val = near_diagonal(np.full(n, 3), n, 1500, dtype, 31)
    return n, off, col, val, kf.vector_x(n, dtype, 32)


def short_rows(dtype):
    return _short_rows(np.dtype(dtype).name)


def tiny(dtype):
    """5 rows, 9 entries: less than one unit of any width"""
    off, col, val = near_diagonal([2, 0, 3, 1, 3], 6, 3, dtype, 5)
    return 6, off, col, val, kf.vector_x(6, dtype, 6)


def tiny_tail_only(dtype):
    """3 entries in 4 rows: as borrowed arrays no whole 16-byte chunk -- the ring kernel is not launched, the tail slot is all"""
    off, col, val = near_diagonal([1, 0, 2, 0], 6, 3, dtype, 7)
    return 6, off, col, val, kf.vector_x(6, dtype, 8)


ALL_WIDTHS = tuple((lanes, 0) for lanes in kf.LANES)
ORDER = ("ru_double", "ru_half", "waves_other", "waves_reversed", "units_descending", "muladd", "plan_order_slots")
TAIL = ("no_tail", "tail_lhs_val_first", "tail_in_row")
REG_ON_OFF = ({"SMH_RING_REGULAR": None}, {"SMH_RING_REGULAR": "0"})

TAIL_WIDTHS = ((1, 0), (8, 0), (64, 0))
WINDOW = ("plan_order_slots", "ru_double")  # (a lane of these plans keeps ONE row: its fma onto +0 is multiply-then-add's number)

RING_CASES = {
    "ragged-owned": RingCase(ragged_with(3), ALL_WIDTHS + ((1, 2), (1, 3), (2, 2)), ORDER),
    "ragged-borrowed-nnz0": RingCase(ragged_with(0), ALL_WIDTHS, ORDER, borrowed=True),
    "ragged-borrowed-nnz1": RingCase(ragged_with(1), ALL_WIDTHS, ORDER + ("no_tail",), borrowed=True),
    "ragged-borrowed-nnz2": RingCase(ragged_with(2), ALL_WIDTHS, ORDER + ("no_tail",), borrowed=True),
    "ragged-borrowed-nnz3": RingCase(ragged_with(3), ALL_WIDTHS, ORDER + ("no_tail",), borrowed=True),
    # ... with lhs on the last two rows only: how the tail's one, two and three entries are rounded shows in the sum
    "ragged-tail-nnz1": RingCase(ragged_with(1), TAIL_WIDTHS, TAIL, borrowed=True, last_rows=2, seed=179),
    "ragged-tail-nnz2": RingCase(ragged_with(2), TAIL_WIDTHS, TAIL, borrowed=True, last_rows=2, seed=120),
    "ragged-tail-nnz3": RingCase(ragged_with(3), TAIL_WIDTHS, TAIL, borrowed=True, last_rows=2, seed=85),
    "ragged-tail-over-two-rows": RingCase(ragged_tail_over_two_rows, TAIL_WIDTHS, TAIL, borrowed=True, last_rows=2, seed=195),
    # 20 000 rows of 32 within 4000 columns of the diagonal: every ring phase is regular
    "window-u32": RingCase(config("k1r-u32"), ((8, 0),), WINDOW, form="u32", env=dict(SMH_RING_COL16="0", SMH_RING_COL12=None)),
    "window-col16": RingCase(config("k1r-col16"), ((8, 0),), WINDOW, form="col16", env=dict(SMH_RING_COL16=None, SMH_RING_COL12="0"),
                             envs=REG_ON_OFF),
    "window-col12": RingCase(config("k1r-col12-auto"), ((8, 0),), WINDOW, form="col12", envs=REG_ON_OFF, dtypes=(F32,), force=False),
    "banded": RingCase(config("k1r-banded"), ((4, 0),), ("plan_order_slots",), bands=4, form="col16", planned=False),
    # the 32768-column ring: 1024 threads, 16 waves.  At 32 lanes a unit is 4 rows, a 64-row phase 16 units: one per wave
    "wide": RingCase(config("k1r-wide"), ((8, 0), (32, 0)), ("waves_other", "waves_reversed"), entries=32768, form="col16", dtypes=(F32,)),
    "mixed-phases": RingCase(kf.mixed_phases, ((2, 0), (8, 0)), ("plan_order_slots", "ru_half")),
    "short-rows": RingCase(short_rows, ((1, 0), (16, 0)), ("units_descending", "waves_other", "waves_reversed", "plan_order_slots", "muladd"), seed=4),
    "tiny": RingCase(tiny, ((1, 0), (4, 0)), ()),
    "tiny-tail-only": RingCase(tiny_tail_only, ((1, 0),), ("no_tail",), borrowed=True),
}


# ---- K1s -------------------------------------------------------------------------------------------------------------------------
STREAM_FORMS = {
    # name: (environment, (xs, direct, value dictionary) knobs, what the getters must report)
    "plain": (dict(SMH_STREAM_C16="0"), (0, -1, -1), dict(coded=False, xs=False, direct=False, vdict=False)),
    "c16": ({}, (0, -1, -1), dict(coded=True, xs=False, direct=False, vdict=False)),
    "xs": ({}, (1, 0, -1), dict(coded=True, xs=True, direct=False, vdict=False)),
    "xd": ({}, (1, 1, 0), dict(coded=True, xs=True, direct=True, vdict=False)),
    "xdv": ({}, (1, 1, -1), dict(coded=True, xs=True, direct=True, vdict=True)),
    # two rows per thread (the SMH_STREAM_RPT tuning knob; the u32 columns): the one form whose epilogue adds a second product to a
    # first, where a fused multiply-add would round differently
    "rpt2": (dict(SMH_STREAM_RPT="2"), (0, -1, -1), dict(coded=False, xs=False, direct=False, vdict=False)),
}
ALL_FORMS = ("plain", "c16", "xs", "xd")


def narrow(n, values=None):
    def build(dtype):
        lens = np.random.default_rng(n).integers(1, 3, n)
        return (n, n) + near_diagonal(lens, n, 300, dtype, n + 1, values)
    return build


def rect_ragged(dtype):
    """7001 x 2503, rows of 0 ... 9 entries anywhere in the row, a run of empty rows"""
    lens = np.random.default_rng(7001).integers(0, 10, 7001)
    lens[3000:3300] = 0
    return (7001, 2503) + near_diagonal(lens, 2503, 2503, dtype, 7002)


TILES_2049 = 2049 * 256 + 3  # the smallest shape with more than 2048 tiles: launch_fold2 takes two workgroups
# name -> (builder -> (n_rows, n_cols, off, col, val), forms, the wrong variants the case must tell apart, seed of its lhs)
STREAM_CASES = {
    "n1": (narrow(1), ALL_FORMS, (), 1),
    "n255": (narrow(255), ALL_FORMS, (), 1),
    "n256": (narrow(256), ALL_FORMS, (), 1),
    "n257": (narrow(257), ALL_FORMS, (), 1),
    "n70001": (narrow(70_001), ALL_FORMS, ("butterfly",), 2),
    "n70001-two-rows-per-thread": (narrow(70_001), ("rpt2",), ("fma",), 1),
    "n70001-five-values": (narrow(70_001, (0.5, -1.25, 3.0, -0.0, 0.1)), ("xdv",), ("butterfly",), 1),
    "tiles2049": (narrow(TILES_2049), ("plain", "xd"), ("butterfly", "one_workgroup_fold"), 1),
    "rect-7001x2503": (rect_ragged, ("plain", "c16"), ("butterfly",), 1),
}


# ---- every other kernel ----------------------------------------------------------------------------------------------------------
GENERIC_VARIANTS = ("seq", "vector", "merge", "colblock", "colfused", "colsplit", "tiled")


def generic_ragged(dtype):
    """6007 x 5001, rows of 0 ... 69 entries, duplicate columns"""
    rng = np.random.default_rng(6007)
    return (6007, 5001) + random_crs(rng, 6007, 5001, rng.integers(0, 70, 6007), dtype, dup=True)


def generic_laplace(dtype):
    n = 23 * 17 * 9
    return (n, n) + oracle.laplace3d(23, 17, 9, dtype)


# name -> (builder, variants, seed of the lhs): the two matrices through every kernel; n_rows on both sides of 2048 (one and two
# workgroups of launch_dot) and of 3 * 2048 (three and four).  Each tells V = 1 and the grid of the other side apart.
GENERIC_CASES = {"ragged-6007x5001": (generic_ragged, GENERIC_VARIANTS, 3), "laplace-23x17x9": (generic_laplace, GENERIC_VARIANTS, 3)}
for _n, _seed in ((2047, 2), (2048, 1), (2049, 3), (6143, 3), (6144, 2), (6145, 6)):
    GENERIC_CASES["n%d" % _n] = (narrow(_n), ("seq", "merge"), _seed)


# ---- the edges every route shares ------------------------------------------------------------------------------------------------
def empty_rows_matrix(dtype):
    """(n_rows, n_cols, off, col, val) 3000 x 3000, rows of 0 ... 9 entries near the diagonal; rows 1000 ... 1299 and the last 200 are
    empty and so are the rows whose drawn length is 0; among the values -0.0, and rows whose only entry is a -0.0"""
    rng = np.random.default_rng(3000)
    lens = rng.integers(0, 10, 3000)
    lens[1000:1300] = 0
    lens[-200:] = 0
    lens[500:520] = 1
    off, col, val = near_diagonal(lens, 3000, 300, dtype, 3001)
    val[5::61] = -0.0
    val[off[500:520]] = -0.0
    return 3000, 3000, off, col, val


# how each route is asked for on that matrix: name -> (variant, ring setting, lanes)
EDGE_ROUTES = {"ring": ("vector", 1, 4), "stream": ("stream", 0, 0), "generic-seq": ("seq", 0, 0), "generic-merge": ("merge", 0, 0),
               "generic-k1": ("vector", 0, 4)}
