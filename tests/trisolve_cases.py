"""The matrices of the triangular-solve tests, shared by tests/test_trisolve_model.py (CPU: every case moves a bit under each
wrong order it can tell apart) and tests/test_trisolve_gpu.py (the device equals the model bit for bit on the same cases)."""
import numpy as np

import sgs_model
import trisolve_model as tm

SMALL_LEVEL_ROWS = 128  # R of the library (asserted against smh_crs_trisolve_levels by the GPU test)

NAMES = ["one", "diagonal", "chain3000", "dense70", "ragged129", "lap24x17", "lap24x17-rb", "lap64x65-rb", "messy", "switch"]


def matrix(name, dtype):
    """(off, col, val, both): ``both`` = the matrix stores both triangles (UPPER solves use it as it is; else its transpose)."""
    if name == "one":
        return tm.from_rows([[(0, 2.5)]], dtype) + (False,)
    if name == "diagonal":
        return tm.from_rows([[(i, 1.5 + 0.01 * i)] for i in range(300)], dtype) + (False,)
    if name == "chain3000":
        return tm.chain(3000, dtype, seed=3) + (False,)
    if name == "dense70":
        return tm.dense_lower(70, dtype, seed=4) + (False,)
    if name == "ragged129":
        return tm.ragged(2 * 64 + 1, dtype, seed=5) + (False,)
    if name.startswith("lap"):
        nx, ny = (24, 17) if name.startswith("lap24x17") else (64, 65)
        off, col, val = sgs_model.lap2d(nx, ny, dtype, seed=6, spread=1.0)
        if name.endswith("-rb"):
            off, col, val = sgs_model.permute_symmetric(off, col, val, sgs_model.red_black(nx, ny))
        return off, col, val, True
    if name == "messy":
        return tm.messy(200, dtype, seed=7) + (True,)
    assert name == "switch"
    return tm.switch_case(SMALL_LEVEL_ROWS, dtype, seed=8) + (False,)


def system(name, dtype, uplo):
    """(off, col, val, b) of the solve with the ``uplo`` triangle."""
    off, col, val, both = matrix(name, dtype)
    if uplo == tm.UPPER and name == "switch":
        off, col, val = tm.reverse(off, col, val)  # (the same levels, mirrored: the transpose has another schedule)
    elif uplo == tm.UPPER and not both:
        off, col, val = tm.transpose(off, col, val)
    b = tm.awkward(np.random.default_rng(len(col) + 11), len(off) - 1, dtype)
    return off, col, val, b


def launches(level_sizes, small_rows):
    """Kernel launches of one solve: a level of more than small_rows rows is one; a run of consecutive smaller levels is one."""
    count, in_run = 0, False
    for size in level_sizes:
        if size > small_rows:
            count, in_run = count + 1, False
        elif not in_run:
            count, in_run = count + 1, True
    return count
