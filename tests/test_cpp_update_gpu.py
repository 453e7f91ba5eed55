"""GPU: element access through the C++ mirror (include/sparsemat.hpp) -- the reference's SparseMatCRS test replayed with
SparseMatCRS::add_to, eye and get (tests/cpp/test_matrix_update.cpp)."""
import os
import subprocess

import pytest

import sparsemat_amd as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_matrix_update(gpu, tmp_path):
    exe = str(tmp_path / "test_matrix_update")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_matrix_update.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
