"""GPU: ilu0, ilu0_refactor, ilu_apply and ILUConjugateGradient through the C++ mirror (include/sparsemat.hpp) on the f64 five-point
system lap2d(12, 9) (tests/cpp/test_ilu.cpp).  Every expected bit is the models' (tests/ilu_model.py, tests/sgs_model.py),
computed here: the mirror solves with the handle's automatic product, which for these short rows is K1s -- bit for bit the
oracle's, with p.Ap out of its epilogue."""
import os
import subprocess

import numpy as np
import pytest

import ilu_model as im
import sgs_model as sg
import sparsemat_amd as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hex64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).view(np.uint64).ravel())


def test_cpp_ilu(gpu, tmp_path):
    tol, iter_max, scale = 1e-10, 200, 0.37
    off, col, val = sg.lap2d(12, 9, np.float64, seed=4, spread=1.0)
    n = len(off) - 1
    b = np.random.default_rng(12).uniform(-1, 1, n)
    w, zp = im.ilu0(off, col, val)
    assert zp is None
    want = sg.sgs_pcg(off, col, val, b, np.zeros(n), tol, iter_max, fused=True, precond=lambda r: im.ilu_apply(off, col, w, r))
    assert 8 < want.iterations < iter_max and np.sqrt(want.r_norm_squared) < tol
    # the mirror solves through AUTO: the expected bits hold while that is K1s (a change of AUTO's choice shows here, not as wrong bits)
    a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    assert a.resolved_variant()[0] == "stream"
    a.scale(scale)  # (the scaled values as the library rounds them)
    w_scaled, _ = im.ilu0(off, col, a.raw_parts()[2])
    data = tmp_path / "case.txt"
    data.write_text("\n".join(["%d %d" % (n, len(col)), " ".join(str(v) for v in off), " ".join(str(v) for v in col), hex64(val), hex64(b),
                               "%r %d %d %r" % (tol, iter_max, want.iterations, scale),
                               hex64(w), hex64(w_scaled), hex64(im.ilu_apply(off, col, w, b)), hex64(want.x)]) + "\n")
    exe = str(tmp_path / "test_ilu")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_ilu.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
