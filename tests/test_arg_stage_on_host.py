"""CPU: the SOURCE of the staging helper of the host/_dev entry-point pairs (sparsemat_amd/csrc/arg_stage.hpp), unchanged, compiled
for the host against a stand-in for the runtime (tests/cpp/arg_stage_on_host/internal.hpp: malloc whose k-th call can be refused,
memcpy, a counted hipDeviceSynchronize, a scripted hipPointerGetAttributes) and run as a program of its own under AddressSanitizer
and UBSan.  Host form: inputs arrive byte for byte, NULL stays NULL, every output goes back once and only in finish(), nothing is
copied for zero bytes, no device-wide sync.  Device form: the caller's pointers as given, no allocation and no copy, one sync when
asked, a pointer on another device refused before any sync.  An allocation refused at the k-th argument, for every k: the status
comes back, no host output is written, nothing stays allocated (the stub's count of live blocks and ASan's leak check)."""
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
    d = tmp_path_factory.mktemp("arg_stage_on_host")
    shutil.copy(os.path.join(ROOT, "sparsemat_amd", "csrc", "arg_stage.hpp"), d / "arg_stage.hpp")
    for name in ("internal.hpp", "arg_stage_on_host.cpp"):
        shutil.copy(os.path.join(ROOT, "tests", "cpp", "arg_stage_on_host", name), d / name)
    out = str(d / "arg_stage_on_host")
    subprocess.check_call([_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", str(d), "-I", os.path.join(ROOT, "include"), str(d / "arg_stage_on_host.cpp"), "-o", out])
    return out


def test_arg_stage_source_under_address_and_ub_sanitizer(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stderr.strip() == "", r.stderr[-3000:]
