"""The matrices of the ILU(0) tests, shared by tests/test_ilu_model.py (CPU: every case moves a bit under each wrong variant it
can tell apart) and tests/test_ilu_gpu.py (the device equals the model bit for bit on the same cases)."""
import numpy as np

import ilu_model as im
import sgs_model
import trisolve_model as tm

SMALL_LEVEL_ROWS = 128  # R of the library (kTriSmallRows)
SLICE = 4               # kIluSlice of csrc/ilu.hip: a group of L lanes factors a row of more than SLICE * L entries in global memory

# name -> the wrong variants of ilu_model.ORDERS the case can tell from the right one.  "descending" needs a row with two
# elimination steps of which the earlier updates the later's multiplier; "fma" and "div_after" need one update.
NAMES = {
    "empty": (), "one": (), "diagonal": (),
    "chain3000": ("fma", "div_after"),
    "dense70": ("fma", "descending", "div_after"),
    "ragged131": ("fma", "descending", "div_after"),
    "ragged290": ("fma", "descending", "div_after"),
    "switch": (),
    "grid130x131": ("fma", "descending", "div_after"),
    "arrow_last": ("fma", "descending", "div_after"),  # (one entry takes 5000 updates: their order shows)
    "arrow_first": ("fma", "div_after"),
    "random2000": ("fma", "descending", "div_after"),
}
for _k in range(len(sgs_model.TABLE)):
    # (table 0 has unit weights: every product with -1 is exact, so only the order of a row's steps shows)
    NAMES["table%d" % _k] = NAMES["table%d-rb" % _k] = ("fma", "descending", "div_after") if sgs_model.TABLE[_k][2] else ("descending",)


def matrix(name, dtype):
    """(off, col, val): rows strictly ascending, every diagonal stored."""
    if name == "empty":
        return np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype)
    if name == "one":
        return tm.from_rows([[(0, 2.5)]], dtype)
    if name == "diagonal":
        return im.diagonal(300, dtype, seed=1)
    if name == "chain3000":  # 3000 levels of one row: one single-workgroup launch
        return im.chain(3000, dtype, seed=2)
    if name == "dense70":  # rows with 0 to 69 elimination steps
        return im.dense(70, dtype, seed=3)
    if name == "ragged131":  # row i: i mod 131 strict-lower entries; rows of 1 to 133 entries: past SLICE * L for L <= 32
        return im.ragged(400, dtype, seed=4)
    if name == "ragged290":  # ... of up to 291 entries: past SLICE * 64 = 256 as well
        return im.ragged(300, dtype, seed=5, period=290)
    if name == "switch":  # 50 small levels, one of R + 1 rows, 49 small levels (lower triangular: divisions only): three launches
        return tm.switch_case(SMALL_LEVEL_ROWS, dtype, seed=8)
    if name == "grid130x131":  # natural levels of 1 .. 130 .. 1 rows: small run, four grid launches, small run
        return sgs_model.lap2d(130, 131, dtype, seed=6, spread=1.0)
    if name.startswith("table"):
        k = int(name[5])
        off, col, val, _, _ = sgs_model.table_case(k, "red_black" if name.endswith("-rb") else "natural")
        return off, col, val.astype(dtype)
    if name.startswith("arrow"):
        # (the last arrow shows a wrong variant in ONE entry, the last diagonal, whose 5000 roundings may end on the same value by
        # chance: the seed is one under which f32 and f64 both end apart)
        return im.arrow(5001, dtype, name == "arrow_first", seed=9)
    assert name == "random2000"
    return im.random_pattern(2000, dtype, seed=9)


_FACTORS = {}


def factor(name, dtype):
    """(w, zero_pivot) of the model on the case, computed once (vector mode: the scalar mode's bits, tests/test_ilu_model.py)."""
    key = name, np.dtype(dtype).name
    if key not in _FACTORS:
        _FACTORS[key] = im.ilu0(*matrix(name, dtype), vector=True)
    return _FACTORS[key]
