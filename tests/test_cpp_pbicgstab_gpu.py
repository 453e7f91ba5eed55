"""GPU: the preconditioner option of BiCGStab through the C++ mirror (include/sparsemat.hpp) on convdiff2d(12, 1.0) with sorted
rows in f64, Jacobi, SGS and ILU(0), both overloads (tests/cpp/test_pbicgstab.cpp).  The body count, the breakdown code, r.r and the
bits of x that the program expects are the model's (tests/pbicgstab_model.py), computed here: the mirror solves with the handle's
automatic product, which for these short rows is K1s -- bit for bit the oracle's.  Each kind is solved to tol 1e-10: the program
checks sqrt(r.r) < 2 tol and the codes."""
import os
import subprocess

import numpy as np
import pytest

import bicgstab_model as bm
import ilu_model as im
import oracle
import pbicgstab_model as pb
import pgmres_model as pm
import sparsemat_amd as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hex64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).view(np.uint64).ravel())


def test_cpp_pbicgstab(gpu, tmp_path):
    tol, iter_max = 1e-10, 400
    off, col, val = pm.sort_rows(*bm.convdiff2d(12, 1.0, np.float64))
    n = 144
    b = oracle.spmv(off, col, val, np.random.default_rng(12).uniform(-1, 1, n))
    w, zp = im.ilu0(off, col, val, vector=True)
    assert zp is None
    # the mirror solves through AUTO: the expected bits hold while that is K1s (a change of AUTO's choice shows here, not as wrong bits)
    assert sm.SparseMatCRS.from_raw_parts(n, n, off, col, val).resolved_variant()[0] == "stream"
    lines = ["%d %d" % (n, len(col)), " ".join(str(v) for v in off), " ".join(str(v) for v in col), hex64(val), hex64(b),
             "%r %d" % (tol, iter_max)]
    for precond in (pm.jacobi(off, col, val), pm.sgs(off, col, val), pm.ilu(off, col, w)):
        want = pb.pbicgstab(off, col, val, b, np.zeros(n), tol, iter_max, precond)
        assert want.converged and want.breakdown == 0 and 3 < want.iterations < iter_max
        lines += ["%d %d" % (want.iterations, want.breakdown), hex64(np.float64(want.r_norm_squared)), hex64(want.x)]
    data = tmp_path / "case.txt"
    data.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "test_pbicgstab")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pbicgstab.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
