"""GPU: BiCGStab through the C++ mirror (include/sparsemat.hpp) on convdiff2d(12, .5) in f64, both overloads
(tests/cpp/test_bicgstab.cpp).  The body count, the breakdown code and the bits of x that the program expects are the model's
(tests/bicgstab_model.py), computed here: the mirror solves with the handle's automatic product, which for these short rows is
K1s -- bit for bit the oracle's."""
import os
import subprocess

import numpy as np
import pytest

import bicgstab_model as bm
import sparsemat_amd as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hex64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).view(np.uint64).ravel())


def test_cpp_bicgstab(gpu, tmp_path):
    tol, iter_max = 1e-10, 200
    off, col, val, b, _ = bm.convdiff_system(12, 0.5, np.float64)
    n = len(b)
    want = bm.bicgstab(off, col, val, b, np.zeros(n), tol, iter_max)
    assert want.converged and want.breakdown == 0 and 8 < want.iterations < iter_max
    # the mirror solves through AUTO: the expected bits hold while that is K1s (a change of AUTO's choice shows here, not as wrong bits)
    assert sm.SparseMatCRS.from_raw_parts(n, n, off, col, val).resolved_variant()[0] == "stream"
    data = tmp_path / "case.txt"
    data.write_text("\n".join(["%d %d" % (n, len(col)), " ".join(str(v) for v in off), " ".join(str(v) for v in col), hex64(val), hex64(b),
                               "%r %d %d %d" % (tol, iter_max, want.iterations, want.breakdown), hex64(want.x)]) + "\n")
    exe = str(tmp_path / "test_bicgstab")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_bicgstab.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
