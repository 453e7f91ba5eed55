"""CPU: the job table of the threading test (tests/thread_jobs.py) and the comparator of its child (tests/thread_child.py) -- the
table is reproducible and read-only, asks for no environment knob, every thread covers it in both passes, and the comparator
turns down each kind of wrong run, naming the thread and the label."""
import hashlib

import numpy as np
import pytest

import thread_child as tc
import thread_jobs as tj
from kernel_forms import CONFIGS


@pytest.fixture(scope="module")
def inputs():
    return tj.build_inputs()


def test_inputs_build_twice_to_the_same_digests_and_are_read_only(inputs):
    assert tj.input_digests(inputs) == tj.input_digests(tj.build_inputs())
    arrays = [a for v in inputs.values() for a in v if isinstance(a, np.ndarray)]
    assert len(arrays) > 100 and not any(a.flags.writeable for a in arrays)
    with pytest.raises(ValueError):
        inputs["sys/laplace24"][4][0] = 1.0


def test_no_job_asks_for_an_environment_knob():
    for name in tj.PRODUCT_CONFIGS:
        assert all(v is None for v in CONFIGS[name].env.values()), name
    assert not tj.qualifies(CONFIGS["k1r-u32"]) and not tj.qualifies(CONFIGS["k1r-col16"])   # (the check can say no)
    names = [j.name for j in tj.job_table()]
    assert len(set(names)) == len(names)
    assert {j.family for j in tj.job_table()} == {"products", "solvers", "builders", "vectors"}
    products = ["product/%s/%s" % (n, tj.NAME[np.dtype(t)]) for n in tj.PRODUCT_CONFIGS for t in CONFIGS[n].dtypes]   # both types where the entry has both
    assert products == [n for n in names if n.startswith("product/")] and len(products) == 2 * len(tj.PRODUCT_CONFIGS) - 1


def test_every_rotation_covers_every_job_in_both_passes():
    n_jobs = len(tj.job_table())
    starts = set()
    for t in range(tj.T):
        first, second = tj.rotation(t, n_jobs)
        assert sorted(first) == sorted(second) == list(range(n_jobs)), t
        assert second == first[::-1] or t, "thread 0 runs the table forwards, then backwards"
        starts.add(first[0])
    assert len(starts) == tj.T   # every thread starts somewhere else


def d(b):
    return hashlib.sha256(b).hexdigest()


SERIAL = [["x", d(b"\x00\x01\x02\x03")], ["iterations", d(tj.i64(11))], ["route", d(b"bucketed")]]


def test_the_comparator_accepts_the_serial_run():
    assert tc.compare_job(SERIAL, [list(p) for p in SERIAL], 5, "j") == []


@pytest.mark.parametrize("what,got,label", [
    ("one flipped bit", [["x", d(b"\x00\x01\x02\x02")], SERIAL[1], SERIAL[2]], "x"),
    ("a missing label", [SERIAL[0], SERIAL[2]], "iterations"),
    ("a swapped route", [SERIAL[0], SERIAL[1], ["route", d(b"general")]], "route"),
    ("an unexpected label", SERIAL + [["extra", d(b"")]], "extra"),
])
def test_the_comparator_rejects(what, got, label):
    bad = tc.compare_job(SERIAL, got, 5, "builder/transpose/band")
    assert len(bad) == 1 and "thread 5" in bad[0] and "builder/transpose/band" in bad[0] and "label %s " % label in bad[0], (what, bad)


BY_PARITY = [dict(transpose_route="bucketed", add_route="same_pattern", apply_route="values_only"),
             dict(transpose_route="general", add_route="general", apply_route="general")]


def own_statuses(t):
    return [("status", tj.i64(3)), ("last_error", tj.expected_last_error(t))] + [(k, v.encode()) for k, v in BY_PARITY[t % 2].items()]


def test_the_comparator_rejects_reads_that_are_another_threads():
    for t in range(tj.T):
        assert tc.compare_statuses(BY_PARITY, own_statuses(t), t) == []
    got = own_statuses(3)
    got[1] = ("last_error", tj.expected_last_error(4))     # the text carries thread 4's number
    bad = tc.compare_statuses(BY_PARITY, got, 3)
    assert len(bad) == 1 and "thread 3" in bad[0] and "label last_error" in bad[0] and "1004" in bad[0] and "1003" in bad[0]
    for label in ("transpose_route", "add_route", "apply_route"):   # an odd thread reads an even thread's route
        got = [(k, (BY_PARITY[0][k].encode() if k == label else v)) for k, v in own_statuses(3)]
        bad = tc.compare_statuses(BY_PARITY, got, 3)
        assert len(bad) == 1 and "thread 3" in bad[0] and "label %s " % label in bad[0], bad
    bad = tc.compare_statuses(BY_PARITY, own_statuses(2)[:-1], 2)
    assert len(bad) == 1 and "thread 2" in bad[0] and "label apply_route is missing" in bad[0]
    bad = tc.compare_statuses(BY_PARITY, [("status", tj.i64(0))] + own_statuses(2)[1:], 2)
    assert len(bad) == 1 and "thread 2" in bad[0] and "label status" in bad[0]


def test_the_comparator_rejects_intervals_that_do_not_overlap():
    busy = {t: (0.1 * t, 10.0 + t) for t in range(tj.T)}
    assert tc.compare_intervals(busy) == []
    busy[6] = (17.5, 18.0)      # after thread 7 has ended (17.0) and after every other thread
    bad = tc.compare_intervals(busy)
    assert len(bad) == 7 and all("thread 6" in b and "busy interval" in b for b in bad)
    assert any("thread 6 and thread 7" in b for b in bad) and any("thread 0 and thread 6" in b for b in bad)
    assert tc.compare_intervals({0: (0.0, 1.0), 1: (1.0, 2.0)}) != []    # one ends as the other starts: serial


class Round:
    """what thread_child.check_handshake reads of a Solving / Arriving thread"""

    def __init__(self, **kw):
        self.error = None
        self.__dict__.update(kw)


def test_the_handshake_check_rejects_wrong_rounds():
    expected = {"jobs": {tc.SOLVE_JOB: [["vec/x", d(b"x")], ["vec/iterations", d(tj.i64(11))]], tc.ARRIVAL_JOB: SERIAL}}
    arriving = Round(results=[list(p) for p in SERIAL])
    good = dict(xs=[d(b"x")] * 4, replays=[3, 3, 0, 0])
    assert tc.check_handshake(2, Round(**good), arriving, expected) == []
    assert tc.check_handshake(4, Round(xs=[d(b"x")], replays=[3]), None, expected) == []     # the thread alone afterwards
    bad = tc.check_handshake(2, Round(**dict(good, xs=[d(b"x"), d(b"y"), d(b"x"), d(b"x")])), arriving, expected)
    assert len(bad) == 1 and "round 2, solve 1" in bad[0] and "label vec/x " in bad[0], bad
    bad = tc.check_handshake(2, Round(**dict(good, replays=[0, 0, 0, 0])), arriving, expected)    # alone, and nothing captured
    assert len(bad) == 1 and "round 2, solve 0" in bad[0] and "label graph_replays " in bad[0], bad
    bad = tc.check_handshake(2, Round(**dict(good, replays=[3, 3, 0, 3])), arriving, expected)    # a capture beside a counted thread
    assert len(bad) == 1 and "round 2, solve 3" in bad[0] and "label graph_replays " in bad[0], bad
    bad = tc.check_handshake(2, Round(**good), Round(results=[SERIAL[0], SERIAL[1], ["route", d(b"general")]]), expected)
    assert len(bad) == 1 and tc.ARRIVAL_JOB in bad[0] and "label route " in bad[0], bad
    bad = tc.check_handshake(2, Round(**good), Round(results=None, error="arriving thread, its first call: HIP error 906"), expected)
    assert bad == ["arriving thread, its first call: HIP error 906"]
