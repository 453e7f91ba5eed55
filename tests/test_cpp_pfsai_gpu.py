"""GPU: the non-symmetric FSAI and the solvers it preconditions through the C++ mirror (include/sparsemat.hpp) on convdiff2d(12, 1.0)
with sorted rows in f64: fsai_ns / fsai_ns_apply, GMRES::solve_fsai (restart 10) and BiCGStab::solve_fsai, both overloads, the pair
passed and made by the solver (tests/cpp/test_pfsai.cpp).  The factors' bits are the model's (tests/fsai_ns_model.py); the body
counts, r.r and the bits of x are those of tests/pfsai_model.py and tests/pbicgstab_model.py fed by the device's own checked
products, computed here: the mirror solves with the handles' automatic products."""
import os
import subprocess

import numpy as np
import pytest

import fsai_ns_cases as nc
import oracle
import sparsemat_amd as sm
from test_pfsai_solvers_gpu import System

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hex64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).view(np.uint64).ravel())


def test_cpp_pfsai(gpu, tmp_path):
    tol, iter_max, restart = 1e-10, 400, 10
    off, col, val = nc.matrix("convdiff12", np.float64)
    n = 144
    b = oracle.spmv(off, col, val, np.random.default_rng(12).uniform(-1, 1, n))
    gl, gu, singular = nc.factor("convdiff12", np.float64)
    assert singular is None
    s = System(off, col, val, b, np.zeros(n), variant="auto", model_pair=(gl, gu))
    lines = ["%d %d" % (n, len(col)), " ".join(str(v) for v in off), " ".join(str(v) for v in col), hex64(val), hex64(b),
             "%r %d %d" % (tol, iter_max, restart), str(len(gl[2])), hex64(gl[2]), str(len(gu[2])), hex64(gu[2])]
    want = s.gmres_model(tol, iter_max, restart)
    assert want.estimates[-1] < tol and want.breakdown == 0 and restart < want.iterations < iter_max and want.cycles > 1
    lines += ["%d %d %d" % (want.iterations, want.cycles, want.breakdown), hex64(np.float64(want.r_norm_squared)), hex64(want.x)]
    want = s.bicgstab_model(tol, iter_max)
    assert want.converged and want.breakdown == 0 and 5 < want.iterations < iter_max
    lines += ["%d %d" % (want.iterations, want.breakdown), hex64(np.float64(want.r_norm_squared)), hex64(want.x)]
    data = tmp_path / "case.txt"
    data.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "test_pfsai")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pfsai.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
