"""GPU: the multi-vector product through the C++ mirror (include/sparsemat.hpp) -- the reference's 34.544 / 20.16 known-answer
matrices from tests/golden/reference_kats.json with k = 3 columns, one of them the reference's vector
(tests/cpp/test_mvp_many.cpp)."""
import json
import os
import subprocess

import pytest

import sparsemat_amd as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mvp_many(gpu, tmp_path):
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")))["cases"]
    lines = []
    for name, expect in (("check_sparsemat_indexlist", "34.544"), ("check_sparsemat_crs", "20.16")):
        case = next(c for c in cases if c["name"] == name)
        crs = case["crs"]
        assert case["expect_mvp"] == [[0, expect]]
        lines.append("%d %d %d" % (crs["n_rows"], crs["n_cols"], len(crs["columns"])))
        lines.append(" ".join(str(v) for v in crs["offset_rows"]))
        lines.append(" ".join(str(v) for v in crs["columns"]))
        lines.append(" ".join(crs["values_bits"]))
        lines.append(" ".join(case["x"]))
        lines.append(expect)
    data = tmp_path / "cases.txt"
    data.write_text("2\n" + "\n".join(lines) + "\n")
    exe = str(tmp_path / "test_mvp_many")
    libdir = os.path.dirname(sm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_mvp_many.cpp"), "-o", exe,
                           "-L", libdir, "-lsparsemat_hip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
