"""CPU: the SOURCE of the eigensolver's host step (sparsemat_amd/csrc/eigsh_host.hpp, free of HIP), unchanged, compiled for the host
into a program of its own (tests/cpp/eigsh_on_host.cpp) under AddressSanitizer and UBSan with -ffp-contract=off, and run on the
inputs of tests/test_eigsh_model.py's Jacobi test -- arrowhead + tridiagonal matrices of m = 2 .. 40 and 128 -- and on the corner
matrices: the sweep count, theta and Y equal eigsh_model.jacobi's BYTE FOR BYTE.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import eigsh_model as em
from sparsemat_amd import build as hip_build
from test_eigsh_model import arrowhead

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clang():
    hipcc = shutil.which(hip_build.hipcc()) or hip_build.hipcc()
    cand = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(cand), "the clang++ that hipcc drives was not found at %s" % cand
    return cand


def hex64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).view(np.uint64).ravel())


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("eigsh_on_host")
    out = str(d / "eigsh_on_host")
    subprocess.check_call([_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "sparsemat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "eigsh_on_host.cpp"), "-o", out])
    return out


def test_host_step_equals_the_model_byte_for_byte(exe, tmp_path):
    mats = [arrowhead(m, m) for m in list(range(2, 41)) + [128]]
    mats += [np.diag([3.0, 1.0, 1.0, 2.0]), np.array([[1e300, 1e-300], [1e-300, -1e300]]), np.array([[0.0, 1.0], [1.0, 0.0]]), np.zeros((3, 3)),
             np.array([[5.0]]), np.array([[1.0, 1e-200], [1e-200, 1.0]]), 1e-160 * arrowhead(6, 1), 1e150 * arrowhead(7, 2)]
    src, dst = tmp_path / "in.txt", tmp_path / "out.txt"
    src.write_text("%d\n" % len(mats) + "".join("%d\n%s\n" % (b.shape[0], hex64(b)) for b in mats))
    r = subprocess.run([exe, str(src), str(dst)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (%d matrices)" % len(mats) in r.stdout and r.stderr.strip() == "", r.stdout[-2000:] + r.stderr[-3000:]
    lines = dst.read_text().split("\n")
    for i, b in enumerate(mats):
        theta, y, sweeps = em.jacobi(b)
        assert np.isfinite(theta).all() and np.isfinite(y).all()
        assert lines[3 * i] == "%d" % sweeps, (i, b.shape, lines[3 * i], sweeps)
        assert lines[3 * i + 1] == hex64(theta), (i, b.shape, "theta")
        assert lines[3 * i + 2] == hex64(y), (i, b.shape, "Y")
