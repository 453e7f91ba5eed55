"""GPU: the reordering operations through the C++ mirror (include/sparsemat.hpp) on the renumbered 24 x 17 grid, against what
the numpy model expects (tests/cpp/test_reorder.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import reorder_model as rm
import sparsemat_amd as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_reorder(gpu, tmp_path):
    n, off, col, val = rm.grid2d(24, 17)
    (off, col, val), _ = rm.renumber(n, off, col, val, seed=7)
    perm, comps, levels = rm.rcm(n, off, col)
    o, c, _ = rm.permute_symmetric(n, off, col, val, perm)
    band = rm.bandwidth(n, o, c)
    assert band[0] == band[1]
    case = tmp_path / "case.txt"
    with open(case, "w") as f:
        for part in ([n, len(col)], off, col, perm, [comps, levels, band[0]]):
            f.write(" ".join(str(int(v)) for v in part) + "\n")
    exe = str(tmp_path / "test_reorder")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_reorder.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
