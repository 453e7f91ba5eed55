"""CPU: the K1s family's stage layout, code bits and tile map (sparsemat_amd/csrc/stream_stage.hpp, the header the kernels' fills, the
code builder and the eligibility statistic call) compiled for the host into a stand-alone program (tests/cpp/stream_stage_on_host.cpp)
and run under AddressSanitizer and UBSan: for hand-written and random interval tables an exact-size stage filled through the chunk map
from an exact-size x holds every column at its entry index, the byte codes survive the offset mask, and every dictionary index
round-trips through both index forms beside every offset."""
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
    d = tmp_path_factory.mktemp("stream_stage_on_host")
    out = str(d / "stream_stage_on_host")
    subprocess.check_call([_clang(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "sparsemat_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "stream_stage_on_host.cpp"),
                           "-o", out])
    return out


def test_stream_stage_layout_and_codes_on_the_host_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout and "ERROR" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
