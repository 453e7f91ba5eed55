"""The models of SparseMatrix::inner_prod's three device routes (tests/inner_prod_model.py), which tests/test_inner_prod_bits_gpu.py
holds the device to bit for bit, checked on the CPU:

  1. the fused multiply-add they are built on against exactly rounded arithmetic (Fraction, tests/test_spmv_order_model.py), inputs
     among them at which multiply-then-add and a sum rounded twice give another result;
  2. fold2 and the ring route against a plain Python loop that walks workgroup -> phase -> wave -> unit -> lane (and grid -> thread
     -> wave) literally, in exactly rounded arithmetic, on plans given by hand;
  3. the row sums the ring phases leave on borrowed, unpadded arrays (ring_sums) against the pure-Python restatement of the lane
     kernels: appending the tail entries to them gives the restatement's rows;
  4. every case of the device test against an exact sum (math.fsum of exact products of f32 data, np.longdouble for f64) within
     gamma(depth) * sum |lhs_i y_i|, gamma(n) = n u / (1 - n u), u the unit roundoff, depth the longest chain of roundings a term
     passes through, counted from the tree -- the standard bound of a sum evaluated in any order, nothing tuned;
  5. for sensitivity: on the data of every device case each wrong variant the case is there to catch moves at least one bit of the
     result.  One listed variant CANNOT be told apart by bits and the test asserts that instead: a fused multiply-add in the K1s
     epilogue with one row per thread is d = fma(lhs, y, +0) = round(lhs * y) + 0 -- the same number; the two-rows-per-thread
     form ("rpt2"), whose second product is added to the first, is the case that tells it."""
import math

import numpy as np
import pytest

import cg_model as cm
import inner_prod_cases as ipc
import inner_prod_model as ipm
import kernel_forms as kf
import oracle
from test_spmv_order_model import BITS, add as x_add, fma as x_fma, lanes_restated, small_lane_matrices

F32, F64 = np.float32, np.float64
BOTH = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
UNIT = {F32: 2.0 ** -24, F64: 2.0 ** -53}


def bits_of(v):
    v = np.asarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64).tolist()


def gamma(n, dtype):
    return n * UNIT[dtype] / (1 - n * UNIT[dtype])


def exact_dot(*factors):
    """(sum of the exact products, sum of their magnitudes), as Python floats / long doubles"""
    if factors[0].dtype == np.float32 and len(factors) == 2:
        p = factors[0].astype(np.float64) * factors[1].astype(np.float64)  # exact: 24 + 24 bits
        return math.fsum(p.tolist()), math.fsum(np.abs(p).tolist())
    p = np.ones(len(factors[0]), np.longdouble)
    for f in factors:
        p = p * f.astype(np.longdouble)
    return p.sum(), np.abs(p).sum()


# ---- 1. the fused multiply-add ---------------------------------------------------------------------------------------------------
@BOTH
def test_fma_is_exactly_rounded(dtype):
    rng = np.random.default_rng(53)
    n = 4000
    a, b, c = (rng.uniform(-2, 2, n) * 2.0 ** rng.integers(-12, 12, n) for _ in range(3))
    c[::7] = -(a * b)[::7] * (1 + rng.uniform(-1, 1, len(c[::7])) * 2.0 ** -20)   # cancellation
    a, b, c = a.astype(dtype), b.astype(dtype), c.astype(dtype)
    a[5::50], b[9::50], c[13::50] = 0.0, -0.0, 0.0
    c[63::100] = -0.0
    # a * b + c a hair below the midpoint of two neighbours of c: multiply-then-add, or a sum rounded first at 53 and then at 24 bits,
    # lands on the midpoint and goes up to the even neighbour
    t = 23 if dtype == F32 else 52
    a[0], b[0], c[0] = 2.0 ** -(t - 5) * (1 + 2.0 ** -t), 1 - 2.0 ** -t, 64 + 2.0 ** -(t - 6)
    got = ipm.fma(a, b, c)
    want = np.array([x_fma(float(p), float(q), float(r), BITS[dtype]) for p, q, r in zip(a, b, c)], dtype)
    assert got.dtype == np.dtype(dtype) and bits_of(got) == bits_of(want)
    assert float(got[0]) == float(c[0]) and float(a[0] * b[0] + c[0]) != float(c[0])   # (the constructed input is what it is said to be)
    assert bits_of(ipm.fma(dtype(-0.0), dtype(1), dtype(0.0))) == bits_of(dtype(0.0))


# ---- 2. the literal walks --------------------------------------------------------------------------------------------------------
def literal_workgroup(acc, bits):
    """256 per-thread values -> thread 0's result: __shfl_down butterfly in each wave (a lane without a partner reads itself), then
    the waves in index order from 0"""
    waves = [list(acc[w * 64:(w + 1) * 64]) for w in range(len(acc) // 64)]
    for v in waves:
        o = 32
        while o:
            v[:] = [x_add(v[l], v[l + o] if l + o < 64 else v[l], bits) for l in range(64)]
            o //= 2
    t = 0.0
    for v in waves:
        t = x_add(t, v[0], bits)
    return t


def literal_fold2(values, bits):
    grid = cm.reduce_blocks(len(values))
    partials = []
    for block in range(grid):
        acc = []
        for thread in range(256):
            s, i = 0.0, block * 256 + thread
            while i < len(values):
                s = x_add(s, float(values[i]), bits)
                i += grid * 256
            acc.append(s)
        partials.append(literal_workgroup(acc, bits))
    acc = []
    for thread in range(256):
        s, i = 0.0, thread
        while i < grid:
            s = x_add(s, partials[i], bits)
            i += 256
        acc.append(s)
    return literal_workgroup(acc, bits)


@BOTH
@pytest.mark.parametrize("count", [1, 2, 255, 257, 1537, 2048, 2049, 4500])
def test_fold2_equals_the_literal_walk(count, dtype):
    vals = np.random.default_rng(count).uniform(-1, 1, count).astype(dtype)
    assert bits_of(ipm.fold2(vals)) == bits_of(dtype(literal_fold2(vals, BITS[dtype])))
    assert cm.reduce_blocks(count) == {2049: 2, 4500: 3}.get(count, 1)


def literal_ring(lhs, y, phase_ptr, phases, lanes, dtype, ring_entries, tail):
    bits = BITS[dtype]
    ru, n_waves = ipm.ring_geometry(lanes, dtype, ring_entries)
    n_blocks = len(phase_ptr) - 1
    parts = []
    for workgroup in range(n_blocks):
        block = (workgroup % 8) * (n_blocks // 8) + workgroup // 8
        dacc = [[0.0] * 64 for _ in range(n_waves)]
        for p in range(int(phase_ptr[block]), int(phase_ptr[block + 1])):
            rb, re = int(phases[p][0]), int(phases[p][1])
            for wave in range(n_waves):
                unit = wave
                while rb + unit * ru < re:
                    for lane in range(ru):
                        r = rb + unit * ru + lane
                        if r < re:
                            dacc[wave][lane] = x_fma(float(lhs[r]), float(y[r]), dacc[wave][lane], bits)
                    unit += n_waves
        parts.append(literal_workgroup([v for wave in dacc for v in wave], bits))
    acc = 0.0
    for r, v, xv in zip(*tail) if tail else ():
        acc = x_fma(float(lhs[r]), float(dtype(v) * dtype(xv)), acc, bits)
    parts.append(acc)
    return parts


HAND_PLANS = [
    # (n_rows, phase_ptr over 8 row ranges, phases): clamped units, a phase of one row, several phases in a range, ranges without any
    (700, [0, 2, 2, 2, 3, 3, 3, 3, 3], [(0, 150), (150, 151), (151, 700)]),
    (1301, [0, 1, 2, 3, 4, 5, 6, 7, 8], [(0, 64), (64, 128), (128, 640), (640, 641), (641, 900), (900, 1100), (1100, 1300), (1300, 1301)]),
]


@BOTH
@pytest.mark.parametrize("lanes", [1, 4, 16, 64])
def test_ring_route_equals_the_literal_walk(lanes, dtype):
    for n, ptr, phases in HAND_PLANS:
        rng = np.random.default_rng(n + lanes)
        lhs, y = ipc.lhs_vector(n, dtype, n), rng.uniform(-1, 1, n).astype(dtype)
        tail = (np.array([n - 2, n - 1, n - 1]), rng.uniform(-1, 1, 3).astype(dtype), rng.uniform(-1, 1, 3).astype(dtype))
        for entries in (16384, 32768) if dtype == F32 else (16384,):
            got = ipm.ring_partials(lhs, y, np.array(ptr), np.array(phases), lanes, dtype, entries, tail)
            want = np.array(literal_ring(lhs, y, ptr, phases, lanes, dtype, entries, tail), dtype)
            assert bits_of(got) == bits_of(want), (n, lanes, entries)
            assert bits_of(ipm.ring_route(lhs, y, np.array(ptr), np.array(phases), lanes, dtype, entries, tail)) == \
                bits_of(dtype(literal_fold2(want, BITS[dtype])))


def test_ring_geometry_and_slots():
    assert [ipm.ring_geometry(lanes, F32, 16384) for lanes in kf.LANES] == [(64, 8), (64, 8), (32, 8), (16, 8), (8, 8), (4, 8), (2, 8)]
    assert [ipm.ring_geometry(lanes, F64, 16384) for lanes in kf.LANES] == [(64, 16), (32, 16), (16, 16), (8, 16), (4, 16), (2, 16), (1, 16)]
    assert ipm.ring_geometry(8, F32, 32768) == (16, 16)
    assert sorted(ipm.ring_slot_block(s, 1536) for s in range(1536)) == list(range(1536))
    assert [ipm.ring_slot_block(s, 1536) for s in (0, 1, 7, 8, 9)] == [0, 192, 1344, 1, 193]


# ---- 3. the ring phases' sums on borrowed, unpadded arrays ---------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("lanes", [1, 4, 32])
def test_ring_sums_are_the_restatement_without_its_tail(lanes, dtype):
    bits, seen = BITS[dtype], 0
    for off, col, val, x in small_lane_matrices(lanes, dtype, 300 + lanes):
        for cut in (0, 1, 2):  # (drop entries of the last row until nnz mod 4 != 0)
            nnz = int(off[-1]) - cut
            if nnz % 4 == 0 or nnz <= int(off[-2]):
                continue
            off2 = off.copy()
            off2[-1] = nnz
            col2, val2 = col[:nnz], val[:nnz]
            limit = nnz & ~3
            y_ring, tail = ipm.ring_sums(off2, col2, val2, x, lanes, borrowed=True)
            whole = oracle.spmv_lanes(off2, col2, val2, x, lanes, tail_from=limit)
            holders = sorted(set(tail[0].tolist()))
            ref = lanes_restated(off2, col2, val2, x, lanes, tail_from=limit, rows=holders)
            out = {r: float(y_ring[r]) for r in holders}
            for r, v, xv in zip(*tail):
                out[int(r)] = x_fma(float(v), float(xv), out[int(r)], bits)
            assert len(tail[0]) == nnz - limit and all(bits_of(dtype(out[r])) == bits_of(ref[r]) == bits_of(whole[r]) for r in holders)
            others = np.setdiff1d(np.arange(len(off2) - 1), holders)
            assert bits_of(y_ring[others]) == bits_of(whole[others])
            assert ipm.ring_sums(off2, col2, val2, x, lanes, borrowed=False)[1] is None
            seen += 1
    assert seen >= 2


# ---- 4. and 5.: the device cases -------------------------------------------------------------------------------------------------
def ring_told(case, dtype, seed=None):
    """the wrong variants (of case.tells) that the case's data tells apart at some width; the model is held to the exact sum on the way"""
    n_cols, off, col, val, x = case.build(dtype)
    n_rows = len(off) - 1
    lhs = case.lhs(n_rows, dtype) if seed is None else ipc.lhs_vector(n_rows, dtype, seed, case.last_rows)
    ptr, phases = ipm.ring_plan_rows(off, col, case.n_blocks, case.entries)
    assert (phases[:, 2] == 1).any() and int(phases[-1, 1]) == n_rows
    told = set()
    for lanes in sorted({w[0] for w in case.widths}):
        y_ring, tail = ipm.ring_sums(off, col, val, x, lanes, case.borrowed)
        got = ipm.ring_route(lhs, y_ring, ptr, phases, lanes, dtype, case.entries, tail)
        exact, scale = exact_dot(lhs, y_ring)
        if tail is not None:
            assert 1 <= len(tail[0]) <= 3
            e2, s2 = exact_dot(lhs[tail[0]], tail[1], tail[2])
            exact, scale = exact + e2, scale + s2
        depth = ipm.ring_depth(ptr, phases, lanes, dtype, case.entries, 0 if tail is None else len(tail[0]))
        assert abs(got - exact) <= gamma(depth, dtype) * scale, (lanes, got, exact, depth)
        for variant in case.tells:
            if variant == "tail_in_row":  # the tail entries appended to their rows' sums, as the plain product does, and no slot of their own
                y_rows = oracle.spmv_lanes(off, col, val, x, lanes, tail_from=int(off[-1]) & ~3)
                other = ipm.ring_route(lhs, y_rows, ptr, phases, lanes, dtype, case.entries)
            else:
                other = ipm.ring_route(lhs, y_ring, ptr, phases, lanes, dtype, case.entries, tail, wrong=(variant,))
            if bits_of(other) != bits_of(got):
                told.add(variant)
    return told


PLANNED = [pytest.param(n, dt, id="%s-%s" % (n, np.dtype(dt).name)) for n, c in ipc.RING_CASES.items() if c.planned for dt in c.dtypes]


@pytest.mark.parametrize("name,dtype", PLANNED)
def test_ring_cases_are_near_the_exact_sum_and_tell_the_wrong_variants(name, dtype):
    case = ipc.RING_CASES[name]
    told = ring_told(case, dtype)
    assert told == set(case.tells), (name, sorted(set(case.tells) - told))


def test_every_ring_variant_has_a_case():
    planned = set().union(*(c.tells for c in ipc.RING_CASES.values() if c.planned))
    assert planned == set(ipm.RING_WRONG) | {"tail_in_row"}
    assert set(ipc.RING_CASES["ragged-tail-over-two-rows"].tells) == set(ipc.TAIL)
    for k in (1, 2, 3):
        assert set(ipc.RING_CASES["ragged-tail-nnz%d" % k].tells) == set(ipc.TAIL)


def stream_wrong(variant, lhs, y, rpt):
    lhs = ipm.pad_lhs(lhs, len(y))
    if variant == "butterfly":  # the __shfl_down butterfly in place of the DPP scan network
        n, tile = len(y), 256 * rpt
        tiles = -(-n // tile)
        terms = np.zeros(tiles * tile, y.dtype)
        terms[:n] = lhs * y
        terms = terms.reshape(tiles, rpt, 256)
        d = np.zeros((tiles, 256), y.dtype)
        for rr in range(rpt):
            d = d + terms[:, rr, :]
        return ipm.fold2(cm.block_sums(d.reshape(-1), from_first=False))
    if variant == "fma":
        n, tile = len(y), 256 * rpt
        tiles = -(-n // tile)
        a, b = np.zeros(tiles * tile, y.dtype), np.zeros(tiles * tile, y.dtype)
        a[:n], b[:n] = lhs, y
        a, b = a.reshape(tiles, rpt, 256), b.reshape(tiles, rpt, 256)
        d = np.zeros((tiles, 256), y.dtype)
        for rr in range(rpt):
            d = ipm.fma(a[:, rr, :], b[:, rr, :], d)
        w = cm.wave_scan_lane63(d.reshape(-1, 64)).reshape(tiles, 4)
        return ipm.fold2(((y.dtype.type(0) + w[:, 0]) + w[:, 1] + w[:, 2]) + w[:, 3])
    assert variant == "one_workgroup_fold"  # the solvers' fold of up to 1024 partials, kept beyond
    return cm.fold_partials(ipm.stream_partials(lhs, y, rpt), False)


def stream_told(name, dtype, seed=None):
    build, forms, tells, case_seed = ipc.STREAM_CASES[name]
    n_rows, n_cols, off, col, val = build(dtype)
    x, lhs = kf.vector_x(n_cols, dtype, 5), ipc.lhs_vector(n_rows, dtype, case_seed if seed is None else seed)
    y = oracle.spmv(off, col, val, x)
    rpt = 2 if forms == ("rpt2",) else 1
    assert "rpt2" not in forms or rpt == 2
    got = ipm.stream_route(lhs, y, rpt)
    exact, scale = exact_dot(lhs, y)
    depth = 1 + rpt + 6 + 4 + ipm.fold2_depth(-(-n_rows // (256 * rpt)))
    assert abs(got - exact) <= gamma(depth, dtype) * scale, (name, rpt)
    if rpt == 2:  # (the handle has no getter for the knob: the device test's bits show that the 512-row tiling ran)
        assert bits_of(ipm.stream_route(lhs, y, 1)) != bits_of(got), name
    if rpt == 1:
        assert bits_of(ipm.stream_partials(lhs, y, 1)) == bits_of(cm.stream_dot_partials(lhs, y))
        # a fused multiply-add onto +0 is the rounded product: not a difference any data can show
        assert bits_of(stream_wrong("fma", lhs, y, 1)) == bits_of(got), name
    return {v for v in tells if bits_of(stream_wrong(v, lhs, y, rpt)) != bits_of(got)}


@BOTH
@pytest.mark.parametrize("name", list(ipc.STREAM_CASES))
def test_stream_cases_are_near_the_exact_sum_and_tell_the_wrong_variants(name, dtype):
    assert stream_told(name, dtype) == set(ipc.STREAM_CASES[name][2]), name


def test_every_stream_variant_has_a_case():
    assert set().union(*(c[2] for c in ipc.STREAM_CASES.values())) == {"butterfly", "fma", "one_workgroup_fold"}
    assert ipc.TILES_2049 == 2049 * 256 + 3 and cm.reduce_blocks(2049) == 2 and cm.reduce_blocks(2048) == 1


def generic_told(name, dtype, seed=None):
    build, _, case_seed = ipc.GENERIC_CASES[name]
    n_rows, n_cols, off, col, val = build(dtype)
    x, lhs = kf.vector_x(n_cols, dtype, 5), ipc.lhs_vector(n_rows, dtype, case_seed if seed is None else seed)
    y = oracle.spmv(off, col, val, x)  # (on the device: the product of the kernel under test)
    got = ipm.generic_route(lhs, y)
    exact, scale = exact_dot(lhs, y)
    grid, V = cm.reduce_blocks(n_rows), cm.vec_len(dtype)
    assert abs(got - exact) <= gamma(1 + cm.tree_depth(n_rows, grid, V), dtype) * scale, name
    terms = lhs * y
    other_grid = grid - 1 if n_rows % 2048 == 1 else grid + 1  # (what n_rows on the other side of the nearest threshold takes)
    return {"V1": bits_of(cm.device_sum(terms, grid, 1)) != bits_of(got), "grid": bits_of(cm.device_sum(terms, other_grid, V)) != bits_of(got)}


@BOTH
@pytest.mark.parametrize("name", list(ipc.GENERIC_CASES))
def test_generic_cases_are_near_the_exact_sum_and_tell_the_wrong_variants(name, dtype):
    assert generic_told(name, dtype) == {"V1": True, "grid": True}, name


def test_generic_cases_lie_on_both_sides_of_the_grid_thresholds():
    assert [cm.reduce_blocks(n) for n in (2047, 2048, 2049, 6143, 6144, 6145)] == [1, 1, 2, 3, 3, 4]
    assert {cm.reduce_blocks(b(F32)[0]) for b, _, _ in ipc.GENERIC_CASES.values()} == {1, 2, 3, 4}


@BOTH
def test_rows_without_entries_change_no_bit_of_a_finite_result(dtype):
    """what the device's treatment of empty rows rests on: with finite lhs, leaving the empty rows' terms out (lhs := +0 there) gives
    the models' bits -- in all three routes, with -0.0 in lhs and among the values"""
    n_rows, n_cols, off, col, val = ipc.empty_rows_matrix(dtype)
    x, lhs = kf.vector_x(n_cols, dtype, 5), ipc.lhs_vector(n_rows, dtype, 6)
    masked = ipm.zero_empty_rows(lhs, off)
    lens = np.diff(off.astype(np.int64))
    assert (lens[1000:1300] == 0).all() and (lens[-200:] == 0).all() and (masked != lhs).any() and np.signbit(lhs[lens > 0]).any()
    y = oracle.spmv(off, col, val, x)
    assert bits_of(ipm.stream_route(lhs, y)) == bits_of(ipm.stream_route(masked, y))
    assert bits_of(ipm.generic_route(lhs, y)) == bits_of(ipm.generic_route(masked, y))
    ptr, phases = ipm.ring_plan_rows(off, col, ipc.RING_BLOCKS, 16384)
    y4 = oracle.spmv_lanes(off, col, val, x, 4)
    assert bits_of(ipm.ring_route(lhs, y4, ptr, phases, 4, dtype, 16384)) == bits_of(ipm.ring_route(masked, y4, ptr, phases, 4, dtype, 16384))
    last = int(np.flatnonzero(lens)[-1])
    assert bits_of(ipm.stream_route(lhs[:last + 1], y)) == bits_of(ipm.stream_route(masked, y))
