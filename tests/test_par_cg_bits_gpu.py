"""The row-partitioned CG (csrc/par.hip smh_par_cg_solve_vec / smh_par_cg_solve, the pieces at the end of csrc/cg.hip) pinned
BIT FOR BIT to tests/par_cg_model.py's restatement of its block folds: x, r.r (as f64(T)) and the number of entered bodies.  The
blocks share device 0 (PEER backend: the fold slots are host-mapped, the meetings ordered by events).  The other partitioned
tests compare the answer by tolerance or the device with itself; CG corrects itself, so neither sees a block value left out of a
fold, a stale scalar block, a slice summed in the wrong form or a stop taken a body late.  Equal bits do.

What each case is for, its seed, and the proof that it can tell the right order from the wrong ones are in
tests/par_cg_cases.py and tests/test_par_cg_model.py (no GPU needed); the model says what the order is."""
import numpy as np
import pytest

import oracle
import par_cg_cases as pc
import sparsemat_amd as sm
from sparsemat_amd import synth
from test_cg_bits_gpu import assert_result, same
from util import assert_spmv_close

pytestmark = pytest.mark.gpu

DTYPES, IDS = pc.DTYPES, pc.IDS


@pytest.fixture(autouse=True)
def fused_dot_knobs_unset(monkeypatch):
    """(read per call by the library: a case that wants the separate dot sets SMH_CG_FUSED_DOT itself)"""
    monkeypatch.delenv("SMH_CG_FUSED_DOT", raising=False)
    monkeypatch.delenv("SMH_STREAM_RPT", raising=False)


def adopt(case):
    """The case's blocks, each its rows of the global matrix with global columns (as tests/test_par_split_gpu.py slices them),
    adopted with the case's split table."""
    blocks = [sm.SparseMatCRS.from_raw_parts(*blk) for blk in case.blocks()]
    m = sm.SparseMatParLocal.adopt(blocks, case.n, split_rows=case.cuts)
    assert m.split() == case.cuts and m.backend() == "peer" and m.n_local_blocks() == len(case.cuts) - 1
    return m


def solve_vec(m, case, variant, check_every=0, **over):
    b, x = m.vec(host=case.b), m.vec(host=case.x0)
    iters, rr = m.cg_solve_vec(b, x, tol=over.get("tol", case.tol), iter_max=over.get("iter_max", case.iter_max), variant=variant, check_every=check_every)
    assert same(b.download(), case.b)  # (b is read only)
    return x.download(), iters, rr


def solve_host(m, case, variant):
    x = case.x0.copy()
    iters, rr = m.cg_solve(case.b, x, tol=case.tol, iter_max=case.iter_max, variant=variant)
    return x, iters, rr


def variants_of(case):
    """[(variant, SMH_CG_FUSED_DOT or None)]: a fused case is K1s with its epilogue; a separate one the bit-exact one-thread-per-row
    kernel and K1s with the epilogue switched off"""
    return [("stream", None)] if case.fused else [("seq", None), ("stream", "0")]


def check_premise(m, case, variant):
    """the product the model takes from the oracle is the device's bit for bit (SEQ and K1s add in the reference's order)"""
    v = case.b - case.x0
    x, y = m.vec(host=v), m.vec()
    m.mvp_dev(x, y, variant=variant)
    m.synchronize()
    assert same(y.download(), oracle.spmv(*case.parts, v)), (case.name, variant, "product not bit-exact")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("reverse", [False, True], ids=["ascending", "big-block-first"])
def test_block_sizes_and_alignments(gpu, monkeypatch, dtype, reverse):
    """Blocks of 1, 2, 3, 5, 255, 257 and 2051 rows (par_cg_cases.HEIGHTS) in both orders: every tail length, fewer rows than
    lanes, a second tile, a second workgroup, block starts at every residue of a 16-byte vector -- the separate dot of an
    unaligned slice strides over elements -- from x0 = 0 and a random x0, polled every 8 (the default), 3 and 1 bodies, and once
    through the host-vector entry."""
    for fused in (False, True):
        for x0_random in (False, True):
            case = pc.split7(dtype, reverse, fused, x0_random)
            want = case.model()
            assert want.iterations == pc.BODIES
            m = adopt(case)
            for variant, knob in variants_of(case):
                with monkeypatch.context() as mp:
                    if knob is not None:
                        mp.setenv("SMH_CG_FUSED_DOT", knob)
                    check_premise(m, case, variant)
                    for check_every in (0, 3, 1):
                        assert_result(solve_vec(m, case, variant, check_every), want, (case.name, variant, knob, check_every))
                    if x0_random:
                        assert_result(solve_host(m, case, variant), want, (case.name, variant, knob, "host vectors"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_even_split_with_a_remainder_overlap_and_threads(gpu, monkeypatch, dtype):
    """with_sub_matrices(3, 3 * 1024 + 5): R = 1025, blocks 1 and 2 start unaligned, the last block has 1027 rows; the exchange is
    a window and every block has interior rows, so with the overlap on the tile partials of p.Ap come from three launches on two
    streams.  Overlap on / off, issuing threads on / off: every arm is the model's, not merely the other arm's."""
    for fused in (False, True):
        case = pc.even3(dtype, fused)
        want = case.model()
        m = sm.SparseMatParLocal.with_sub_matrices(3, case.n, case.n, *case.parts, device_ids=[0, 0, 0])
        assert m.split() == pc.EVEN_CUTS == case.cuts and m.exchange_mode("auto")[0] == "window"
        for b in range(3):
            a, e = m.interior(b, "stream")
            assert a < e, (b, a, e)
        for variant, knob in variants_of(case):
            with monkeypatch.context() as mp:
                if knob is not None:
                    mp.setenv("SMH_CG_FUSED_DOT", knob)
                check_premise(m, case, variant)
                for threads in (1, 0):
                    m.set_threads(threads)
                    for overlap in (True, False):
                        m.set_overlap(overlap)
                        assert_result(solve_vec(m, case, variant, 4), want, (case.name, variant, knob, threads, overlap))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_all_gather_exchange(gpu, monkeypatch, dtype):
    """The tridiagonal matrix plus the coupling (i, n - 1 - i): every block references every other, the exchange resolves to the
    all-gather."""
    for fused in (False, True):
        case = pc.gather3(dtype, fused)
        want = case.model()
        m = sm.SparseMatParLocal.with_sub_matrices(3, case.n, case.n, *case.parts, device_ids=[0, 0, 0])
        assert m.split() == pc.GATHER_CUTS and m.exchange_mode("auto")[0] == "allgather"
        for variant, knob in variants_of(case):
            with monkeypatch.context() as mp:
                if knob is not None:
                    mp.setenv("SMH_CG_FUSED_DOT", knob)
                check_premise(m, case, variant)
                assert_result(solve_vec(m, case, variant), want, (case.name, variant, knob))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_past_the_caps(gpu, dtype):
    """One matrix, three bodies: block 0 (1 048 576 + 2051 rows) asks for 514 workgroups in the update sweep, capped at 512, and
    gets 514 in launch_dot; block 1 (524 288 + 1027 rows) leaves 2053 tile partials, which launch_fold2 takes with two
    workgroups; blocks 1 and 2 start unaligned.  The smallest heights at which those branches are taken."""
    assert pc.cg_model.reduce_blocks(pc.CAPS_CUTS[1]) == 514 > pc.cg_model.CG_GRID_CAP
    assert pc.cg_model.reduce_blocks((pc.CAPS_CUTS[2] - pc.CAPS_CUTS[1] + 255) // 256) == 2
    m = None
    for fused in (False, True):
        case = pc.caps(dtype, fused)
        m = m or adopt(case)
        variant = "stream" if fused else "seq"
        assert_result(solve_vec(m, case, variant), case.model(), (case.name, variant))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stops_in_exactly_the_converging_body(gpu, dtype):
    """tol lies between sqrt(rr_4) and every earlier norm (chosen from the model's own rr_list): iterations == 4 on every
    block -- one x, one r.r -- and x is body 4's, whether the poll comes every 3 or every 16 bodies."""
    for fused in (False, True):
        case = pc.stop_case(dtype, fused)
        want = case.model()
        assert want.iterations == pc.STOP_BODY
        m = adopt(case)
        variant = "stream" if fused else "seq"
        for check_every in (3, 16):
            assert_result(solve_vec(m, case, variant, check_every), want, (case.name, check_every))
            assert_result(solve_vec(m, case, variant, check_every, iter_max=pc.STOP_BODY), want, (case.name, check_every, "iter_max = the stopping body"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_iter_max_and_the_reference_breakdown(gpu, dtype):
    """iter_max 5 polled every 3 (the limit falls inside the second batch), 2 polled every 8, 0 (x untouched, the initial r.r
    reported); b = 0: alpha = 0 / 0, NaN to iter_max like the reference (NaN equals NaN in `same`)."""
    for iter_max, check_every in ((5, 3), (2, 8), (0, 8)):
        case = pc.limits_case(dtype, iter_max)
        want = case.model()
        assert want.iterations == iter_max
        got = solve_vec(adopt(case), case, "seq", check_every)
        assert_result(got, want, (case.name, check_every))
        if iter_max == 0:
            assert same(got[0], case.x0) and same(np.float64(got[2]), np.float64(want.rr0))
    z = np.zeros(pc.N7, dtype)
    case = pc.limits_case(dtype, 5).with_(b=z, x0=z, tol=1e-6)
    want = case.model()
    assert want.iterations == 5 and np.isnan(want.x).all() and np.isnan(want.r_norm_squared)
    m = adopt(case)
    for variant in ("seq", "stream"):
        assert_result(solve_vec(m, case, variant, 2), want, ("b = 0", variant))


def test_solves_are_reproducible(gpu):
    """Two solves on one handle, and two handles with the same split: equal bits (the scalar blocks, the fold slots and the
    handle's own p are left over from the first solve)."""
    for case, variant in ((pc.split7(np.float32, False, True, True), "stream"), (pc.split7(np.float64, True, False, True), "seq")):
        m1, m2 = adopt(case), adopt(case)
        first = solve_vec(m1, case, variant, 4)
        for other in (solve_vec(m1, case, variant, 4), solve_vec(m1, case, variant, 5), solve_vec(m2, case, variant, 4), solve_host(m2, case, variant)):
            assert other[1] == first[1] and same(np.float64(other[2]), np.float64(first[2])) and same(other[0], first[0])
        assert_result(first, case.model(), case.name)


def test_auto_kernel_per_block(gpu):
    """test_adopted_device_born_blocks' blocks (40 000 x 32, f32, 4 blocks born on the device): AUTO is the ring kernel, whose
    order of additions is not the oracle's, so the model takes every product from the device's own m.mvp_dev -- held to the parity
    bound against the oracle first.  The matrix is not symmetric; the recurrence is defined all the same (the model's iterates
    are finite: tests/test_par_cg_model.py).  Five bodies, overlap on and off."""
    case = pc.auto_blocks()
    r = pc.AUTO_N // pc.AUTO_BLOCKS
    blocks = [synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_BANDED, pc.AUTO_N, pc.AUTO_K, np.float32, k * r, (k + 1) * r) for k in range(pc.AUTO_BLOCKS)]
    m = sm.SparseMatParLocal.adopt(blocks, pc.AUTO_N)
    assert m.split() == case.cuts and m.exchange_mode("auto")[0] == "window"
    seen = {}

    def product(v):
        v = np.ascontiguousarray(v, np.float32)
        key = v.tobytes()
        if key not in seen:
            x, y = m.vec(host=v), m.vec()
            m.mvp_dev(x, y)
            m.synchronize()
            got = y.download()
            assert_spmv_close(got, *case.parts, v, "partitioned solver's product, AUTO")
            seen[key] = got
        return seen[key].copy()

    want = case.model(product=product)
    assert all(b.resolved_variant()[0] == "vector" and b.ring_plan()[2] for b in blocks)
    assert want.iterations == pc.AUTO_BODIES and np.isfinite(want.x).all()
    for overlap in (True, False):
        m.set_overlap(overlap)
        assert_result(solve_vec(m, case, "auto", 2), want, ("auto", overlap))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_block_without_rows(gpu, monkeypatch, dtype):
    """check_split admits split[k + 1] == split[k]: the empty block multiplies nothing, contributes +0 to every fold (its
    fused dot has no tile: the separate dot of no terms) and takes the same decisions as the others."""
    for fused in (False, True):
        case = pc.empty_block(dtype, fused)
        want = case.model()
        m = adopt(case)
        for variant, knob in variants_of(case):
            with monkeypatch.context() as mp:
                if knob is not None:
                    mp.setenv("SMH_CG_FUSED_DOT", knob)
                assert_result(solve_vec(m, case, variant, 4), want, (case.name, variant, knob))
