"""CPU: the functions of K1r's 24-bit value code (sparsemat_amd/csrc/ring_val24.hpp, the header the encoder kernels and the ring
kernel call) compiled for the host into a stand-alone program (tests/cpp/ring_val24_on_host.cpp) and run under AddressSanitizer and
UBSan: all 2^24 integers round-trip bit for bit at E = -23 (against the synthetic generator's formula), 0 and -21, quadruples pack and
unpack with the extremes in every position, and -0.0, NaN, +-Inf, subnormals, 0.1f, values one past the range or with a bit below E,
and exponents outside the bound are refused."""
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
    d = tmp_path_factory.mktemp("ring_val24_on_host")
    out = str(d / "ring_val24_on_host")
    subprocess.check_call([_clang(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "sparsemat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ring_val24_on_host.cpp"), "-o", out])
    return out


def test_ring_val24_code_on_the_host_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout and "ERROR" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
