"""CPU: the SOURCE of the partition's arithmetic (sparsemat_amd/csrc/par_plan.hpp), unchanged, compiled for the host and run as a
program of its own under AddressSanitizer and UBSan (tests/cpp/par_plan_on_host.cpp).  Every (n_blocks, n_rows) with 1 <= n_blocks <= 6
and n_blocks <= n_rows <= 40, the reference's partition and split tables with empty blocks, random column intervals: every column a
block references outside its own rows lies in exactly one recv_range, no range touches the receiver's rows, what q receives from src
is what src sends to q, plan_summary's maximum is a count by hand; split_by_nnz against its definition by linear scan (all rows
empty, one heavy row), every block keeping a row; the block lookup inverts block_rows for every row; the longest run of clean tiles
against brute force on every pattern of up to 10 tiles; the rounding of an interior to a kernel's granularity never leaves the
interior and gives nothing when it would give the whole block.  All arrays are allocated at their exact size."""
import os
import shutil
import subprocess

import pytest

from sparsemat_amd import build as hip_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clang():
    hipcc = shutil.which(hip_build.hipcc()) or hip_build.hipcc()
    cand = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(cand), "the clang++ that hipcc drives was not found at %s" % cand
    return cand


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("par_plan_on_host") / "par_plan_on_host")
    subprocess.check_call([_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "sparsemat_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "par_plan_on_host.cpp"), "-o", out])
    return out


def test_par_plan_source_under_address_and_ub_sanitizer(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stderr.strip() == "", r.stderr[-3000:]


def test_par_plan_header_is_host_only():
    """Nothing of the GPU runtime or of RCCL: the header and the issuing threads' header include only the standard library and the C ABI."""
    for name in ("par_plan.hpp", "par_issue.hpp"):
        with open(os.path.join(ROOT, "sparsemat_amd", "csrc", name)) as f:
            includes = [line.split()[1] for line in f if line.startswith("#include")]
        assert includes and all(i.startswith("<") and "hip" not in i and "rccl" not in i or i == '"../../include/sparsemat_hip.h"' for i in includes), includes
