"""The program tests/test_threads_gpu.py starts: `python tests/thread_child.py warm|cold JSON_PATH`.

INTEGRATION.md: "a handle is not thread-safe; distinct handles may be used from distinct threads."  A thread that uses only handles
and vectors it created must get, bit for bit, what one thread gets.

warm: the main thread loads the library, runs every job of tests/thread_jobs.py once -- each held to its reference outside the
      library (Job.verify) --, writes the digests of the results to JSON_PATH, and then starts T threads behind a barrier; thread t
      runs the table twice (rotated by t * ceil(J / T), then in reverse order), after the status calls of thread_jobs.status_calls.
cold: the same threaded run with no serial pass before it: the main thread only loads the library and counts the devices, so every
      kernel family, occupancy query, function-attribute opt-in and lazily read knob is met first by T threads at once.  What to
      expect is read from JSON_PATH, the warm child's serial pass in another process.

cold, after its workers have ended: the handshake of the library's capture guard (handshake()): a thread that solves alone captures
      and replays; a second thread whose first call is DenseVec.from_vec arrives meanwhile; beside it nothing is captured; a
      thread alone afterwards captures again; every x is the serial one.

After the joins: every threaded result equals the serial one label by label, byte for byte; every thread read its own last error
and routes; the live bytes of the pool are back where they were; and every thread's busy interval overlaps every other's (the run
was not serial in secret).  Exit 0: all held.  1: something differed.  3: a thread was still running at the time limit -- the
program says what each thread was doing and leaves at once, starting nothing more on the device.

No torch in this process: the library alone initialises the runtime."""
import ctypes as C
import gc
import hashlib
import json
import os
import sys
import threading
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import thread_jobs as tj  # noqa: E402

JOIN_SECONDS = 200        # all threads together; the parent's own limit is 300
STATUS = "statuses"       # the name under which a thread's status calls are kept among its results


def digest(b):
    return hashlib.sha256(b).hexdigest()


def digests(results):
    return [[label, digest(b)] for label, b in results]


# ---- the comparator (tests/test_thread_jobs_host.py feeds it wrong runs) ---------------------------------------------------------
def compare_job(expected, got, thread, job):
    """expected, got: [[label, digest]] -- the same labels in the same order with the same bytes.  Returns the complaints, each
    naming the thread, the job and the label."""
    bad = []
    e_labels, g_labels = [l for l, _ in expected], [l for l, _ in got]
    for l in e_labels:
        if l not in g_labels:
            bad.append("thread %d, job %s: label %s is missing" % (thread, job, l))
    for l in g_labels:
        if l not in e_labels:
            bad.append("thread %d, job %s: label %s was not expected" % (thread, job, l))
    if not bad and e_labels != g_labels:
        bad.append("thread %d, job %s: labels in another order, first at %s" % (thread, job, next(a for a, b in zip(e_labels, g_labels) if a != b)))
    want = dict(map(tuple, expected))
    for l, d in got:
        if l in want and want[l] != d:
            bad.append("thread %d, job %s: label %s differs from the serial run" % (thread, job, l))
    return bad


def compare_statuses(by_parity, got, thread):
    """got: [(label, bytes)] of thread_jobs.status_calls(thread).  The last error must carry this thread's number; the routes must
    be those of this thread's parity (by_parity[t % 2]: {label: text} of the serial pass)."""
    bad = []
    if dict(got).get("status") != tj.i64(3):   # SMH_ERR_INDEX_RANGE: refused, a status
        bad.append("thread %d, job %s: label status is not the refusal's" % (thread, STATUS))
    d = {l: (b.decode(errors="replace") if isinstance(b, bytes) else b) for l, b in got}
    want = dict(by_parity[thread % 2], last_error=tj.expected_last_error(thread).decode())
    for label in ("last_error", "transpose_route", "add_route", "apply_route"):
        if label not in d:
            bad.append("thread %d, job %s: label %s is missing" % (thread, STATUS, label))
        elif d[label] != want[label]:
            bad.append("thread %d, job %s: label %s reads %r, this thread's own is %r" % (thread, STATUS, label, d[label], want[label]))
    return bad


def compare_intervals(busy):
    """busy: {thread: (first job's start, last job's end)}.  Every two threads' intervals must overlap."""
    bad = []
    for a in sorted(busy):
        for b in sorted(busy):
            if a < b and not (busy[a][0] < busy[b][1] and busy[b][0] < busy[a][1]):
                bad.append("thread %d and thread %d, label busy interval: %.3f .. %.3f and %.3f .. %.3f do not overlap" % ((a, b) + tuple(busy[a]) + tuple(busy[b])))
    return bad


# ---- the run ---------------------------------------------------------------------------------------------------------------------
def pool_stats(sm):
    kept, live = C.c_size_t(), C.c_size_t()
    sm._lib.check(sm.lib().smh_pool_stats(C.byref(kept), C.byref(live)))
    return kept.value, live.value


def pool_live(sm):
    gc.collect()
    sm._lib.check(sm.lib().smh_pool_trim())
    return pool_stats(sm)[1]


def status_texts(results):
    return {l: b.decode() for l, b in results if l != "status"}


def serial_pass(inp, jobs, sm):
    """every job once on the main thread, each held to its reference -> (expected, complaints)"""
    expected, bad = {"jobs": {}, "statuses": {}, "inputs": tj.input_digests(inp)}, []
    for parity in (0, 1):
        got = tj.status_calls(inp, sm, parity, lambda: None)
        assert dict(got)["status"] == tj.i64(sm._lib.SMH_ERR_INDEX_RANGE) and dict(got)["last_error"] == tj.expected_last_error(parity), got
        expected["statuses"][str(parity)] = {l: t for l, t in status_texts(got).items() if l != "last_error"}
    for label, route in expected["statuses"]["0"].items():   # a getter that reads the same for both parities could not show a shared one
        assert route != expected["statuses"]["1"][label], (label, route)
    for job in jobs:
        t0 = time.monotonic()
        try:
            results = job.run(inp, sm)
            t1 = time.monotonic()
            expected["jobs"][job.name] = digests(results)
            if job.verify:
                job.verify(inp, tj.Got(results), sm)
            print("serial %-40s run %6.3f s  reference %6.3f s" % (job.name, t1 - t0, time.monotonic() - t1), flush=True)
        except Exception:
            bad.append("serial pass, job %s: %s" % (job.name, traceback.format_exc(limit=6)))
            print(bad[-1], flush=True)
        gc.collect()
    return expected, bad


class Worker(threading.Thread):
    def __init__(self, t, inp, jobs, sm, barrier):
        super().__init__(name="worker-%d" % t, daemon=True)
        self.t, self.inp, self.jobs, self.sm, self.barrier = t, inp, jobs, sm, barrier
        self.doing, self.results, self.intervals, self.error = "waiting to start", [], [], None

    def run(self):
        try:
            self.barrier.wait(60)
            self.doing = STATUS
            self.results.append((0, STATUS, tj.status_calls(self.inp, self.sm, self.t, lambda: self.barrier.wait(60))))
            for n_pass, order in enumerate(tj.rotation(self.t, len(self.jobs))):
                for k in order:
                    job = self.jobs[k]
                    self.doing = "pass %d, job %s" % (n_pass, job.name)
                    t0 = time.monotonic()
                    got = job.run(self.inp, self.sm)
                    self.intervals.append((job.name, t0, time.monotonic()))
                    self.results.append((n_pass, job.name, digests(got)))
            self.doing = "done"
        except Exception:
            self.error = "thread %d, %s: %s" % (self.t, self.doing, traceback.format_exc(limit=6))


def threaded_pass(inp, jobs, sm, expected):
    bad = []
    barrier = threading.Barrier(tj.T)
    workers = [Worker(t, inp, jobs, sm, barrier) for t in range(tj.T)]
    t_start = time.monotonic()
    for w in workers:
        w.start()
    deadline = t_start + JOIN_SECONDS
    for w in workers:
        w.join(max(0.0, deadline - time.monotonic()))
    if any(w.is_alive() for w in workers):
        for w in workers:
            print("thread %d: %s after %.0f s: %s" % (w.t, "STILL RUNNING" if w.is_alive() else "finished", time.monotonic() - t_start, w.doing), flush=True)
        os._exit(3)
    busy = {}
    for w in workers:
        if w.error:
            bad.append(w.error)
            continue
        busy[w.t] = (w.intervals[0][1], w.intervals[-1][2])
        print("thread %d busy %.3f .. %.3f s (%d jobs)" % (w.t, busy[w.t][0] - t_start, busy[w.t][1] - t_start, len(w.intervals)), flush=True)
        for n_pass, name, got in w.results:
            if name == STATUS:
                bad += compare_statuses([expected["statuses"]["0"], expected["statuses"]["1"]], got, w.t)
            elif name in expected["jobs"]:
                bad += compare_job(expected["jobs"][name], got, w.t, "%s (pass %d)" % (name, n_pass))
        ran = sorted(name for _, name, _ in w.results if name != STATUS)
        if ran != sorted(2 * [j.name for j in jobs]):
            bad.append("thread %d did not run every job twice" % w.t)
    if len(busy) == tj.T:
        bad += compare_intervals(busy)
    print("threaded pass: %.3f s" % (time.monotonic() - t_start), flush=True)
    return bad


# ---- a thread that arrives while another captures (cold only) ----------------------------------------------------------------------
HANDSHAKE_ROUNDS = 4
SOLVE_JOB, ARRIVAL_JOB = "solver/cg/laplace24/stream", "vector/f32/4097"


class Solving(threading.Thread):
    """Solves alone first -- the only thread the library counts, so the batch is captured and replayed --, then goes on solving
    while the second thread arrives, and once more after that thread was counted: no capture beside it.  Every x is the serial one."""

    def __init__(self, inp, sm, alone_only=False):
        super().__init__(daemon=True)
        self.inp, self.sm, self.alone_only = inp, sm, alone_only
        self.first_done, self.other_counted, self.done = threading.Event(), threading.Event(), threading.Event()
        self.doing, self.xs, self.replays, self.error = "waiting to start", [], [], None

    def run(self):
        try:
            sm = self.sm
            n, off, col, val, b, x0 = self.inp["sys/laplace24"][:6]
            a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
            a.prepare("stream")
            s = sm.ConjugateGradient(0.0, tj.ITER_MAX, "stream", check_every=tj.CHECK_EVERY)   # thread_jobs.solver_job's "vec" entry
            bd = sm.DenseVec.from_vec(b)

            def solve(what):
                self.doing = what
                xd = sm.DenseVec.from_vec(x0)
                s.solve(a, bd, xd)
                self.xs.append(digest(xd.to_numpy().tobytes()))
                self.replays.append(s.graph_replays)
            solve("the solve alone")
            self.first_done.set()
            if not self.alone_only:
                for k in range(200):                      # (the other thread arrives within a few of these)
                    solve("solve %d while the other thread arrives" % k)
                    if k >= 2 and self.other_counted.is_set():
                        break
                assert self.other_counted.is_set(), "the other thread never made its first call"
                solve("the solve beside a counted thread")
            self.doing = "done"
        except Exception:
            self.error = "solving thread, %s: %s" % (self.doing, traceback.format_exc(limit=6))
        finally:
            self.first_done.set()
            self.done.set()


class Arriving(threading.Thread):
    """Its first call into the library is DenseVec.from_vec -- a create, a synchronous memset and copy -- while the other thread solves;
    then a vector job.  It stays (counted) until the solving thread has finished."""

    def __init__(self, inp, job, sm, solving):
        super().__init__(daemon=True)
        self.inp, self.job, self.sm, self.solving = inp, job, sm, solving
        self.doing, self.results, self.error = "waiting to start", None, None

    def run(self):
        try:
            self.doing = "its first call, DenseVec.from_vec"
            v = self.inp["vec/f32/4097"][0]
            back = self.sm.DenseVec.from_vec(v).to_numpy()
            self.solving.other_counted.set()
            assert back.tobytes() == v.tobytes(), "DenseVec.from_vec did not keep the vector"
            self.doing = "job " + self.job.name
            self.results = digests(self.job.run(self.inp, self.sm))
            self.doing = "waiting for the solving thread"
            assert self.solving.done.wait(60), "the solving thread did not finish"
            self.doing = "done"
        except Exception:
            self.error = "arriving thread, %s: %s" % (self.doing, traceback.format_exc(limit=6))
        finally:
            self.solving.other_counted.set()


def join_all(threads, seconds, t_start):
    deadline = time.monotonic() + seconds
    for w in threads:
        w.join(max(0.0, deadline - time.monotonic()))
    if any(w.is_alive() for w in threads):
        for w in threads:
            print("%s: %s after %.0f s: %s" % (type(w).__name__, "STILL RUNNING" if w.is_alive() else "finished", time.monotonic() - t_start, w.doing), flush=True)
        os._exit(3)


def check_handshake(round_, solving, arriving, expected):
    """the complaints of one round; tests/test_thread_jobs_host.py feeds it wrong rounds"""
    bad = [w.error for w in (solving, arriving) if w is not None and w.error]
    if bad:
        return bad
    want = dict(map(tuple, expected["jobs"][SOLVE_JOB]))["vec/x"]
    for k, x in enumerate(solving.xs):
        if x != want:
            bad.append("handshake round %d, solve %d: label vec/x differs from the serial run" % (round_, k))
    if solving.replays[0] <= 0:
        bad.append("handshake round %d, solve 0: label graph_replays is %d for a thread alone in the library: nothing was captured" % (round_, solving.replays[0]))
    if arriving is not None:
        if solving.replays[-1] != 0:
            bad.append("handshake round %d, solve %d: label graph_replays is %d beside a counted thread" % (round_, len(solving.xs) - 1, solving.replays[-1]))
        bad += compare_job(expected["jobs"][ARRIVAL_JOB], arriving.results, 1, "%s (handshake round %d)" % (ARRIVAL_JOB, round_))
    return bad


def handshake(inp, jobs, sm, expected):
    """Only where no living thread is counted by the library (csrc/internal.hpp, "host threads and graph capture"): the cold child,
    whose main thread has made no counted call, after its workers have ended.  HANDSHAKE_ROUNDS times two fresh threads: one solves
    alone (and captures), the other makes its first call beside it; then one fresh thread alone again, which must capture again --
    threads that have ended are counted no longer."""
    bad, t_start = [], time.monotonic()
    job = next(j for j in jobs if j.name == ARRIVAL_JOB)
    for r in range(HANDSHAKE_ROUNDS + 1):
        solving = Solving(inp, sm, alone_only=r == HANDSHAKE_ROUNDS)
        solving.start()
        arriving = None
        if not solving.first_done.wait(60):
            join_all([solving], 0, t_start)
        if r < HANDSHAKE_ROUNDS:
            arriving = Arriving(inp, job, sm, solving)
            arriving.start()
        join_all([w for w in (solving, arriving) if w], 60, t_start)
        bad += check_handshake(r, solving, arriving, expected)
        print("handshake round %d: graph replays of the solves %s" % (r, solving.replays), flush=True)
        if bad:
            break
    print("handshake: %.3f s" % (time.monotonic() - t_start), flush=True)
    return bad


def main(mode, json_path):
    assert mode in ("warm", "cold")
    assert not [k for k in os.environ if k.startswith("SMH_")], "the child runs without SMH_* variables: the library reads them lazily"
    t_begin = time.monotonic()
    inp = tj.build_inputs()
    jobs = tj.job_table()
    import util
    util.BUCKET_LOG_FILE = False
    import sparsemat_amd as sm
    n = C.c_int(0)
    sm._lib.check(sm.lib().smh_device_count(C.byref(n)))
    assert n.value > 0, "no HIP device"
    print("%s: %d jobs, inputs built in %.1f s" % (mode, len(jobs), time.monotonic() - t_begin), flush=True)
    bad = []
    if mode == "warm":
        live0 = pool_live(sm)
        t0 = time.monotonic()
        expected, bad = serial_pass(inp, jobs, sm)
        print("serial pass: %.3f s with its references" % (time.monotonic() - t0), flush=True)
        with open(json_path, "w") as f:
            json.dump(expected, f)
        jobs = [j for j in jobs if j.name in expected["jobs"]]
        if pool_live(sm) != live0:
            bad.append("serial pass: %d live bytes in the pool, %d before" % (pool_live(sm), live0))
    else:
        with open(json_path) as f:
            expected = json.load(f)
        assert expected["inputs"] == tj.input_digests(inp), "the inputs differ from the warm child's"
        live0 = pool_stats(sm)[1]     # (no trim: smh_pool_stats touches no device, and the main thread stays out of the library's count)
    bad += threaded_pass(inp, jobs, sm, expected)
    if mode == "cold" and not bad:
        bad += handshake(inp, jobs, sm, expected)
    live = pool_live(sm)
    if live != live0:
        bad.append("after the threads: %d live bytes in the pool, %d before them" % (live, live0))
    for line in bad[:40]:
        print("FAIL " + line, flush=True)
    print("%s: %d complaints, %.1f s in all" % (mode, len(bad), time.monotonic() - t_begin), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.stdout.flush()
    code = main(sys.argv[1], sys.argv[2])
    sys.stdout.flush()
    sys.exit(code)
