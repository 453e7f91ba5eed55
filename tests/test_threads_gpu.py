"""INTEGRATION.md's threading contract -- "distinct handles may be used from distinct threads" -- on the device: eight host threads,
each on handles and vectors of its own, run the whole job table of tests/thread_jobs.py (every product form, the solvers, the
builders, the vector kernels, the per-thread getters) and must get, bit for bit, what one thread gets.  The work is done by
tests/thread_child.py in a process of its own (no torch in it): first with a serial pass in front, in which every job is held to
its reference outside the library ("warm"), then with the library's first use of everything made by eight threads at once
("cold").

One limit is the runtime's: on ROCm 7.2 a hipMemcpy, hipMemset or hipDeviceSynchronize from any host thread is refused while another
thread captures a graph, hipStreamCaptureModeThreadLocal or not, and invalidates that capture.  So the solvers capture only while
one host thread is using the library (csrc/internal.hpp, "host threads and graph capture"); the cold child ends with a thread that
arrives while a lone thread captures."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_child(mode, json_path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SMH_")}   # (the library reads its knobs lazily, with getenv)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "thread_child.py"), mode, json_path], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        raise AssertionError("the %s child was still running after 300 s:\n%s" % (mode, out[-3000:]))
    print(r.stdout[-6000:])
    assert r.returncode == 0, "the %s child left with %d:\n%s" % (mode, r.returncode, r.stdout[-3000:])
    assert "busy" in r.stdout


def test_distinct_handles_from_distinct_threads(gpu, tmp_path):
    json_path = str(tmp_path / "serial.json")
    run_child("warm", json_path)
    run_child("cold", json_path)     # (not reached when the warm child failed: nothing else is started then)
