"""GPU: mixed precision through the C++ mirror (include/sparsemat.hpp) on convdiff2d(24, 1.0) with sorted rows in f64: cast<U>() on
SparseMatCRS and DenseVec, and IterativeRefinement with GMRES(30) + ILU(0) and with BiCGSTAB + FSAI inside, both overloads, the f32
matrix and its factors passed and made by the solver (tests/cpp/test_refine.cpp).  The cast's bits are numpy's; the outer steps, the
inner bodies, r.r, the code and the bits of x are those of tests/refine_model.py fed by the device's own checked products, computed
here: the mirror solves with the handles' automatic products."""
import os
import subprocess

import numpy as np
import pytest

import refine_cases as rc
import refine_model as rm
import sparsemat_amd as sm
from test_refine_gpu import Device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hex64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).view(np.uint64).ravel())


def hex32(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).view(np.uint32).ravel())


def test_cpp_refine(gpu, tmp_path):
    gmres, bicgstab = Device(rc.BY_NAME["gmres30+ilu"], "auto", "auto"), Device(rc.BY_NAME["bicgstab+fsai"], "auto", "auto")
    off, col, val, b = gmres.off, gmres.col, gmres.val, gmres.b
    assert np.array_equal(val, bicgstab.val) and np.array_equal(b, bicgstab.b) and not gmres.x0.any()
    n, tol = len(b), gmres.case.tol
    lines = ["%d %d" % (n, len(col)), " ".join(str(v) for v in off), " ".join(str(v) for v in col), hex64(val), hex32(rm.cast(val, np.float32)), hex64(b),
             hex32(rm.cast(b, np.float32)), "%r" % tol]
    for d in (gmres, bicgstab):
        want = d.model()
        assert want.code == 0 and want.outer >= 2 and np.sqrt(want.rr) < tol
        lines += ["%d %d %d" % (want.outer, want.iterations, want.code), hex64(np.float64(want.rr)), hex64(want.x)]
    data = tmp_path / "case.txt"
    data.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "test_refine")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_refine.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
