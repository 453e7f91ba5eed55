"""CPU: the SOURCE of the device-memory caching layer (sparsemat_amd/csrc/pool.hip), unchanged, compiled for the host against a
stand-in for the runtime (tests/cpp/pool_on_host/internal.hpp: malloc under a byte budget per "device", a current device per
thread) and run from eight threads under ThreadSanitizer: no block handed out twice, the per-thread byte accounting back at 0,
nothing live or kept or leaked at the end, the refuse-trim-retry path taken -- and no report of a data race."""
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
    d = tmp_path_factory.mktemp("pool_on_host")
    shutil.copy(os.path.join(ROOT, "sparsemat_amd", "csrc", "pool.hip"), d / "pool.inc")
    for name in ("internal.hpp", "pool_on_host.cpp"):
        shutil.copy(os.path.join(ROOT, "tests", "cpp", "pool_on_host", name), d / name)
    out = str(d / "pool_on_host")
    subprocess.check_call([_clang(), "-std=c++20", "-O1", "-g", "-fsanitize=thread", "-pthread", "-I", str(d), str(d / "pool_on_host.cpp"), "-o", out])
    return out


def test_pool_source_from_eight_threads_under_thread_sanitizer(exe):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SMH_")}   # (SMH_POOL_MAX_BYTES would change the layer's cap)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert "ThreadSanitizer" not in r.stderr and r.stderr.strip() == "", r.stderr[-3000:]
