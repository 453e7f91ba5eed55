"""GPU: fsai, fsai_apply and FSAIConjugateGradient through the C++ mirror (include/sparsemat.hpp) on the f64 five-point system
lap2d(12, 9) (tests/cpp/test_fsai.cpp).  Every expected bit is the models' (tests/fsai_model.py, tests/sgs_model.py), computed
here: the mirror multiplies through the handles' automatic product, which for these short rows is K1s -- bit for bit the oracle's,
with p.Ap out of its epilogue."""
import os
import subprocess

import numpy as np
import pytest

import fsai_model as fm
import oracle
import sgs_model as sg
import sparsemat_amd as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hex64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).view(np.uint64).ravel())


def test_cpp_fsai(gpu, tmp_path):
    tol, iter_max = 1e-10, 200
    off, col, val = sg.lap2d(12, 9, np.float64, seed=4, spread=1.0)
    n = len(off) - 1
    b = np.random.default_rng(12).uniform(-1, 1, n)
    goff, gcol, gval, bad = fm.fsai(off, col, val)
    assert bad is None
    g, gt = (goff, gcol, gval), fm.transpose(goff, gcol, gval)
    precond = lambda r: fm.fsai_apply(g, gt, r, oracle.spmv)
    want = sg.sgs_pcg(off, col, val, b, np.zeros(n), tol, iter_max, fused=True, precond=precond)
    assert 8 < want.iterations < iter_max and np.sqrt(want.r_norm_squared) < tol
    # the mirror goes through AUTO: the expected bits hold while that is K1s (a change of AUTO's choice shows here, not as wrong bits)
    a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    dg, dgt, _ = a.fsai()
    assert a.resolved_variant()[0] == dg.resolved_variant()[0] == dgt.resolved_variant()[0] == "stream"
    data = tmp_path / "case.txt"
    data.write_text("\n".join(["%d %d %d" % (n, len(col), len(gcol)), " ".join(str(v) for v in off), " ".join(str(v) for v in col), hex64(val), hex64(b),
                               "%r %d %d" % (tol, iter_max, want.iterations),
                               hex64(gval), hex64(gt[2]), hex64(precond(b)), hex64(want.x)]) + "\n")
    exe = str(tmp_path / "test_fsai")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_fsai.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
