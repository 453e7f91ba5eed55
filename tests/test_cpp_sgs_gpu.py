"""GPU: the triangular solve, the SGS application and SGSConjugateGradient through the C++ mirror (include/sparsemat.hpp) on the
f64 five-point system lap2d(12, 9) (tests/cpp/test_sgs.cpp).  The level counts, the body count and every expected bit are the
models' (tests/trisolve_model.py, tests/sgs_model.py), computed here: the mirror solves with the handle's automatic product,
which for these short rows is K1s -- bit for bit the oracle's, with p.Ap out of its epilogue."""
import os
import subprocess

import numpy as np
import pytest

import sgs_model as sg
import sparsemat_amd as sm
import trisolve_model as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hex64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).view(np.uint64).ravel())


def test_cpp_sgs(gpu, tmp_path):
    tol, iter_max = 1e-10, 200
    off, col, val = sg.lap2d(12, 9, np.float64, seed=4, spread=1.0)
    n = len(off) - 1
    b = np.random.default_rng(12).uniform(-1, 1, n)
    want = sg.sgs_pcg(off, col, val, b, np.zeros(n), tol, iter_max, fused=True)
    assert 8 < want.iterations < iter_max and np.sqrt(want.r_norm_squared) < tol
    # the mirror solves through AUTO: the expected bits hold while that is K1s (a change of AUTO's choice shows here, not as wrong bits)
    assert sm.SparseMatCRS.from_raw_parts(n, n, off, col, val).resolved_variant()[0] == "stream"
    lower = tm.trisolve(off, col, val, b, tm.LOWER, False)
    upper_unit = tm.trisolve(off, col, val, b, tm.UPPER, True)
    data = tmp_path / "case.txt"
    data.write_text("\n".join(["%d %d" % (n, len(col)), " ".join(str(v) for v in off), " ".join(str(v) for v in col), hex64(val), hex64(b),
                               "%r %d %d %d %d" % (tol, iter_max, want.iterations, tm.levels(off, col, tm.LOWER)[1], tm.levels(off, col, tm.UPPER)[1]),
                               hex64(want.x), hex64(lower), hex64(upper_unit), hex64(sg.sgs_apply(off, col, val, b))]) + "\n")
    exe = str(tmp_path / "test_sgs")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_sgs.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
