"""CPU: the SOURCE of the issuing threads of a partitioned handle (sparsemat_amd/csrc/par_issue.hpp), unchanged, compiled for the host
and run as a program of its own (tests/cpp/par_issue_on_host.cpp) under ThreadSanitizer, and once more under AddressSanitizer and
UBSan.  n = 1, 2 and 8 blocks: hundreds of phases back to back, a gap in which the workers go to sleep, more phases -- every fn(k)
exactly once per phase and on one thread per k, block 0 on the caller; a failing k hands its status and its own thread's text to the
caller and the next phase runs; a throwing fn is a status, nothing terminates; a start hook that refuses the m-th thread, for each m,
leaves everything on the caller with no thread kept and nobody waited for; destruction while the workers sleep and while they spin."""
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


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"], ids=["tsan", "asan_ubsan"])
def test_par_issue_source_under_sanitizers(tmp_path, sanitizer):
    out = str(tmp_path / "par_issue_on_host")
    subprocess.check_call([_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "sparsemat_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "par_issue_on_host.cpp"), "-o", out])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stderr.strip() == "", r.stderr[-3000:]
