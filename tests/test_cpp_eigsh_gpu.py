"""GPU: Lanczos through the C++ mirror (include/sparsemat.hpp) on tridiag(-1, d_i, -1) of n = 100 in f64, k = 4, m = 20, LARGEST, every
overload (tests/cpp/test_eigsh.cpp): one converged case.  The counts, the breakdown code and the bits of the values, the estimates
and the vectors that the program expects are the model's (tests/eigsh_model.py), computed here: the mirror solves with the handle's
automatic product, which for these short rows is K1s -- bit for bit the oracle's."""
import os
import subprocess

import numpy as np
import pytest

import eigsh_model as em
import sparsemat_amd as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hex64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).view(np.uint64).ravel())


def test_cpp_lanczos(gpu, tmp_path):
    n, k, ncv, which, tol, restart_max = 100, 4, 20, em.LARGEST, 1e-10, 200
    off, col, val = em.tridiag_sym(n, np.float64, seed=0)
    start = em.start_vector(n, np.float64, seed=2)
    want = em.eigsh(off, col, val, start, k, ncv, which, tol, restart_max)
    assert want.n_conv == k and want.breakdown == 0 and 0 < want.restarts < restart_max
    # the mirror solves through AUTO: the expected bits hold while that is K1s (a change of AUTO's choice shows here, not as wrong bits)
    assert sm.SparseMatCRS.from_raw_parts(n, n, off, col, val).resolved_variant()[0] == "stream"
    data = tmp_path / "case.txt"
    data.write_text("\n".join(["%d %d" % (n, len(col)), " ".join(str(v) for v in off), " ".join(str(v) for v in col), hex64(val), hex64(start),
                               "%d %d %d %r %d %d %d %d %d" % (k, ncv, which, tol, restart_max, want.n_conv, want.restarts, want.products, want.breakdown),
                               hex64(want.values), hex64(want.estimates), hex64(want.vectors)]) + "\n")
    exe = str(tmp_path / "test_eigsh")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_eigsh.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
