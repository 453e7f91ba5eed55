"""CPU: the SOURCE of the K1m kernel (sparsemat_amd/csrc/spmv_many.hip) compiled for the host against a stand-in for a workgroup
(tests/cpp/hip_on_host/internal.hpp: 256 threads and a barrier) and run under AddressSanitizer and UBSan -- bit for bit the
storage-order sum per column, padding columns +0, no access outside exact-size arrays -- for the KT = 4 body and the KT = 8 one."""
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
    d = tmp_path_factory.mktemp("k1m_on_host")
    shutil.copy(os.path.join(ROOT, "sparsemat_amd", "csrc", "spmv_many.hip"), d / "spmv_many.inc")
    shutil.copy(os.path.join(ROOT, "tests", "cpp", "hip_on_host", "internal.hpp"), d / "internal.hpp")
    shutil.copy(os.path.join(ROOT, "tests", "cpp", "k1m_on_host.cpp"), d / "k1m_on_host.cpp")
    out = str(d / "k1m_on_host")
    subprocess.check_call([_clang(), "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-I", str(d), str(d / "k1m_on_host.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("args", [[], ["kt8"]], ids=["kt4", "kt8"])
def test_k1m_source_on_the_host_under_sanitizers(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout and "ERROR" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
