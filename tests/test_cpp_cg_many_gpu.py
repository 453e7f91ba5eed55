"""GPU: MultiVec's per-column BLAS-1 and ConjugateGradient::solve_many through the C++ mirror (include/sparsemat.hpp) on a small
SPD system with k = 3 right-hand sides of different scale (tests/cpp/test_cg_many.cpp).  The iteration counts the program
expects are the model's (tests/cg_many_model.py), computed here."""
import os
import subprocess

import numpy as np
import pytest

import cg_many_model
import cg_model
import sparsemat_amd as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hex64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).view(np.uint64).ravel())


def test_cpp_cg_many(gpu, tmp_path):
    n, k, tol, iter_max = 300, 3, 1e-10, 200
    off, col, val = cg_model.tridiag(n, np.float64, seed=6)
    rng = np.random.default_rng(6)
    B = rng.uniform(-1, 1, (k, n)) * np.array([1.0, 1e-3, 1e-6])[:, None]
    want = cg_many_model.cg_many(off, col, val, B, np.zeros((k, n)), tol, iter_max)
    assert len(set(want.iterations.tolist())) == 3 and want.iterations.max() < iter_max   # the columns stop in different bodies
    data = tmp_path / "case.txt"
    data.write_text("\n".join(["%d %d %d" % (n, len(col), k), " ".join(str(v) for v in off), " ".join(str(v) for v in col), hex64(val)] +
                              [hex64(row) for row in B] + ["%r %d" % (tol, iter_max), " ".join(str(v) for v in want.iterations)]) + "\n")
    exe = str(tmp_path / "test_cg_many")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cg_many.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
