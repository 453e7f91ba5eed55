"""GPU: the multicolour ordering through the C++ mirror (include/sparsemat.hpp) on the renumbered 24 x 17 grid (seed 1) and the
clique of 65 vertices (seed 0: a colour per vertex, one past the mask window), against what the numpy model expects
(tests/cpp/test_color.cpp)."""
import os
import subprocess

import pytest

import color_model as cm
import sparsemat_amd as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_color(gpu, tmp_path):
    cases = [("grid_24x17_renumbered", 1), ("clique_65", 0)]
    case = tmp_path / "cases.txt"
    with open(case, "w") as f:
        f.write("%d\n" % len(cases))
        for name, seed in cases:
            n, off, col = cm.case(name)
            want = cm.expected(name, seed)
            for part in ([n, len(col), seed], off, col, want["colors"], want["perm"], [want["n_colors"], want["n_rounds"]]):
                f.write(" ".join(str(int(v)) for v in part) + "\n")
    exe = str(tmp_path / "test_color")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_color.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
