"""The two summation-order models of the oracle -- oracle.spmv_lanes (K1 / K1r) and oracle.spmv_merge (K2), which
tests/test_spmv_order_gpu.py and tests/test_solver_kernels_gpu.py hold the device to bit for bit -- checked on the CPU:

  1. against a slow restatement in pure Python, written from the kernels' header comments with exactly rounded arithmetic (Fraction,
     then one rounding to nearest even at 24 or 53 bits; signed zeros by the IEEE rules), bit for bit, on small inputs: every row
     length 0 ... 8 lanes + 5 at every start s mod 4, for every lanes, both value types, with and without the K1r tail; merge on
     matrices of up to 200 rows with tiles of 512, 1024 and 2048 items, rows that cross several tiles among them;
  2. against the reference's storage-order sum (util.assert_spmv_close, the suite's parity bound) on every matrix the device tests
     launch;
  3. for sensitivity: on every one of those cases each wrong variant of a model (oracle.LANES_WRONG, oracle.MERGE_WRONG, other lanes,
     other tiles) changes the bits of at least one row -- except where the case CANNOT tell the variant apart, which BLIND_LANES /
     merge_can_tell state with the reason, and where the test then asserts that no row changes (so the exceptions stay exact)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import kernel_forms as kf
import oracle
from kernel_forms import same
from util import assert_spmv_close

F32, F64 = np.float32, np.float64
BITS = {F32: 24, F64: 53}
EXP_RANGE = {24: (-126, 127), 53: (-1022, 1023)}


# ---- exactly rounded arithmetic: values are Python floats that hold numbers of the format exactly ----------------------------
def round_to(q, bits):
    """the Fraction q != 0 (a dyadic rational: sums and products of binary floating-point numbers) rounded to nearest, ties to
    even, at `bits` significant bits (normal range only)"""
    num, k = abs(q.numerator), q.denominator.bit_length() - 1
    assert q.denominator == 1 << k
    drop = num.bit_length() - bits          # low bits of the numerator that do not fit
    if drop <= 0:
        n, drop = num, 0
    else:
        n, rem, half = num >> drop, num & ((1 << drop) - 1), 1 << (drop - 1)
        if rem > half or (rem == half and n & 1):
            n += 1  # (n == 2 ** bits then: the next binade's first number, which ldexp gives exactly)
    e = num.bit_length() - 1 - k            # 2 ** e <= |q| < 2 ** (e + 1)
    lo, hi = EXP_RANGE[bits]
    assert lo <= e < hi, "out of the normal range: not what these tests are about"
    r = math.ldexp(n, drop - k)
    return -r if q < 0 else r


def neg(v):
    return math.copysign(1.0, v) < 0


def add(a, b, bits):
    q = Fraction(a) + Fraction(b)
    if q == 0:
        return -0.0 if neg(a) and neg(b) and a == 0 and b == 0 else 0.0  # x + (-x) = +0; (-0) + (-0) = -0
    return round_to(q, bits)


def mul(a, b, bits):
    q = Fraction(a) * Fraction(b)
    if q == 0:
        return -0.0 if neg(a) != neg(b) else 0.0
    return round_to(q, bits)


def fma(a, b, c, bits):
    q = Fraction(a) * Fraction(b) + Fraction(c)
    if q == 0:
        exact_zero_product = a == 0 or b == 0
        return -0.0 if exact_zero_product and c == 0 and (neg(a) != neg(b)) and neg(c) else 0.0
    return round_to(q, bits)


def test_round_to_is_the_formats_rounding():
    rng = np.random.default_rng(3)
    for _ in range(300):
        a, b, c = (float(v) for v in rng.uniform(-2, 2, 3) * 2.0 ** rng.integers(-20, 20, 3))
        q = Fraction(a) * Fraction(b) + Fraction(c)
        assert round_to(q, 53) == float(q)                                  # (int / int is correctly rounded in Python)
        a32, b32 = float(F32(a)), float(F32(b))
        assert round_to(Fraction(a32) * Fraction(b32), 24) == float(F32(a32) * F32(b32))  # (a 48-bit product is exact in f64: one rounding)
    assert round_to(Fraction(2 ** 24 + 1), 24) == 2.0 ** 24 and round_to(Fraction(2 ** 24 + 3), 24) == 2.0 ** 24 + 4  # ties to even
    assert round_to(Fraction(2 ** 25 - 1), 24) == 2.0 ** 25                # carries into the next binade
    assert str(fma(-0.0, 1.0, 0.0, 24)) == "0.0" and str(fma(-0.0, 1.0, -0.0, 24)) == "-0.0" and str(fma(1.0, 1.0, -1.0, 24)) == "0.0"
    assert str(add(-0.0, -0.0, 24)) == "-0.0" and str(add(-0.0, 0.0, 24)) == "0.0" and str(mul(-1.0, 0.0, 24)) == "-0.0"


# ---- K1 / K1r restated -------------------------------------------------------------------------------------------------------
def lane_slots(j, lanes, pairs, n_slots):
    """the entry slots (counted from the row's 4-aligned start) that lane j of the group takes, in the order it takes them"""
    out = []
    if pairs:  # f64: two 16-byte pieces of two entries per pass of 4 lanes slots
        for first in range(0, n_slots, 4 * lanes):
            out += [first + 2 * j, first + 2 * j + 1, first + 2 * lanes + 2 * j, first + 2 * lanes + 2 * j + 1]
    else:      # f32: the 16-byte chunks j, j + lanes, j + 2 lanes, ...
        for chunk in range(j, (n_slots + 3) // 4, lanes):
            out += [4 * chunk, 4 * chunk + 1, 4 * chunk + 2, 4 * chunk + 3]
    return out


def lanes_restated(off, col, val, x, lanes, tail_from=None, rows=None):
    """{row: y[row]} for the rows asked for (default: all)"""
    bits = BITS[val.dtype.type]
    nnz = int(off[-1])
    limit = nnz if tail_from is None else tail_from   # what the streaming kernel may touch
    y = {}
    for r in (range(len(off) - 1) if rows is None else rows):
        s, e = int(off[r]), int(off[r + 1])
        s_k, e_k = min(s, limit), min(e, limit)
        first = s_k - s_k % 4                       # the chunk grid is anchored at element 0 of the arrays
        sums = []
        for j in range(lanes):
            acc = 0.0
            for slot in lane_slots(j, lanes, bits == 53, e_k - first):
                k = first + slot
                if s_k <= k < e_k:
                    acc = fma(float(val[k]), float(x[col[k]]), acc, bits)
            sums.append(acc)
        o = lanes // 2
        while o:
            sums = [add(sums[j], sums[j ^ o], bits) for j in range(lanes)]
            o //= 2
        out = sums[0]
        for k in range(max(s, limit), e):           # the tail kernel: one entry after the other, onto the stored result
            out = fma(float(val[k]), float(x[col[k]]), out, bits)
        y[r] = val.dtype.type(out)
    return y


def small_lane_matrices(lanes, dtype, seed):
    """matrices of at most 200 rows that hold, between them, every row length 0 ... 2 * 4 * lanes + 5 and every start s mod 4 (up to 8 lanes: every pair of
    them; beyond: every pair within 6 of 0, 4 lanes and 8 lanes entries, the other lengths at one start each): before each row comes a row of 0 ... 3 entries that moves the start to the residue wanted.  Some stored +0.0 and -0.0, one x of 0."""
    rng = np.random.default_rng(seed)
    lengths = range(8 * lanes + 6)
    pairs = [(length, mod) for length in lengths for mod in range(4)]
    if lanes > 8:  # (the restatement costs ~10 us per entry) every pair where a pass or a chunk begins or ends, else one start each
        edge = [n for n in lengths if min(abs(n - m) for m in (0, 4 * lanes, 8 * lanes)) <= 6]
        pairs = [(n, m) for n in edge for m in range(4)] + [(n, (n // 3) % 4) for n in lengths if n not in edge]
        assert {n for n, _ in pairs} == set(lengths) and {m for n, m in pairs if n > 4 * lanes + 6} == {0, 1, 2, 3}
    out = []
    for i in range(0, len(pairs), 100):
        lens, at = [], 0
        for length, mod in pairs[i:i + 100]:
            lens += [(mod - at) % 4, length]
            at = (mod + length) % 4
        off = np.zeros(len(lens) + 1, np.uint32)
        np.cumsum(lens, out=off[1:])
        assert len(lens) <= 200 and all((int(off[2 * k + 1]) % 4, int(off[2 * k + 2] - off[2 * k + 1])) == (m, n)
                                        for k, (n, m) in enumerate(pairs[i:i + 100]))
        n_cols = 50
        col = rng.integers(0, n_cols, int(off[-1]), dtype=np.uint32)
        val = rng.uniform(-1, 1, len(col)).astype(dtype)
        val[rng.integers(0, len(val), len(val) // 40)] = 0.0
        val[rng.integers(0, len(val), len(val) // 40)] = -0.0
        x = rng.uniform(-1, 1, n_cols).astype(dtype)
        x[3] = 0.0
        out.append((off, col, val, x))
    return out


def bits_of(a):
    return int(np.asarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.uint64))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("lanes", kf.LANES)
def test_lane_model_equals_the_restatement(lanes, dtype):
    for off, col, val, x in small_lane_matrices(lanes, dtype, 100 + lanes):
        nnz = int(off[-1])
        got = oracle.spmv_lanes(off, col, val, x, lanes)
        ref = lanes_restated(off, col, val, x, lanes)
        bad = [r for r in ref if bits_of(got[r]) != bits_of(ref[r])]
        assert not bad, (lanes, bad[:5], [(got[r], ref[r]) for r in bad[:5]])
        # the K1r tail: only the rows that hold entries from nnz & ~3 on may differ from the above, and they are restated again
        limit = nnz & ~3
        tail_rows = [r for r in range(len(off) - 1) if off[r + 1] > limit]
        assert (nnz % 4 == 0) == (not tail_rows)
        got_t = oracle.spmv_lanes(off, col, val, x, lanes, tail_from=limit)
        ref_t = lanes_restated(off, col, val, x, lanes, tail_from=limit, rows=tail_rows)
        assert all(bits_of(got_t[r]) == (bits_of(ref_t[r]) if r in ref_t else bits_of(got[r])) for r in range(len(off) - 1)), (lanes, tail_rows)


# ---- K2 restated -------------------------------------------------------------------------------------------------------------
def merge_restated(off, col, val, x, tile=2048):
    """spmv_merge.hip's header, step by step: the merged list is, row after row, the row's entries and then its end."""
    bits = BITS[val.dtype.type]
    n_rows = len(off) - 1
    items = []
    for r in range(n_rows):
        items += [("entry", k, r) for k in range(int(off[r]), int(off[r + 1]))] + [("end", None, r)]
    y = [0.0] * n_rows
    carries = []                                        # per tile: (the row it leaves open or None, what it holds of that row)
    for t0 in range(0, len(items), tile):
        threads = tile // 8
        open_part, finished, first = [], [], []
        for t in range(threads):
            running, mine = 0.0, None
            for kind, k, r in items[t0 + 8 * t:min(t0 + 8 * t + 8, t0 + tile)]:
                if kind == "entry":
                    running = add(running, mul(float(val[k]), float(x[col[k]]), bits), bits)
                else:
                    if mine is None:
                        mine = (r, running)             # may miss what earlier threads hold of this row
                    else:
                        y[r] = running
                    running = 0.0
            open_part.append(running)
            finished.append(mine is not None)
            first.append(mine)
        # segmented inclusive scan inside each wave of 64: after the step with distance o a lane holds the sum of up to 2 o lanes
        sv, sf = list(open_part), list(finished)
        o = 1
        while o < 64:
            pv, pf = list(sv), list(sf)
            for t in range(threads):
                if t % 64 >= o:
                    if not pf[t]:
                        sv[t] = add(pv[t - o], pv[t], bits)
                    sf[t] = pf[t] or pf[t - o]
            o *= 2
        incl, before_wave = [], []
        prefix = 0.0                                    # what the earlier waves hold of the row open at this wave's start
        for w in range(threads // 64):
            before_wave.append(prefix)
            for t in range(64 * w, 64 * w + 64):
                incl.append(sv[t] if sf[t] else add(prefix, sv[t], bits))
            last = 64 * w + 63
            prefix = sv[last] if sf[last] else add(prefix, sv[last], bits)
        for t in range(threads):
            if first[t] is not None:
                carry_in = incl[t - 1] if t % 64 else before_wave[t // 64]
                y[first[t][0]] = add(carry_in, first[t][1], bits)
        nxt = items[t0 + tile][2] if t0 + tile < len(items) else None
        carries.append((nxt, incl[-1]))
    t = 0
    while t < len(carries):
        r = carries[t][0]
        u = t
        acc = 0.0
        while u < len(carries) and carries[u][0] == r:
            acc = add(acc, carries[u][1], bits)
            u += 1
        if r is not None:
            y[r] = add(acc, y[r], bits)
        t = u
    return np.array(y, val.dtype)


def small_merge_matrices(dtype):
    rng = np.random.default_rng(77)
    out = []
    for lens in ([0] * 3 + [9, 0, 1, 2, 600, 3, 0, 0, 1500, 7] + list(rng.integers(0, 12, 120)),   # rows over several threads, waves, tiles
                 [2300] + list(rng.integers(0, 5, 150)) + [0] * 40 + [1],                            # a row over two tile boundaries (tile 1024)
                 [7] * 192,                                                                         # rows end on the tile boundaries (8 items each)
                 list(rng.integers(0, 30, 60))):                                                    # a single tile of 2048
        n_cols = 40
        off = np.zeros(len(lens) + 1, np.uint32)
        np.cumsum(lens, out=off[1:])
        col = rng.integers(0, n_cols, int(off[-1]), dtype=np.uint32)
        val = rng.uniform(-1, 1, len(col)).astype(dtype)
        val[::31] = 0.0
        val[7::53] = -0.0
        x = rng.uniform(-1, 1, n_cols).astype(dtype)
        assert len(lens) <= 200
        out.append((off, col, val, x))
    return out


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("tile", [512, 1024, 2048])
def test_merge_model_equals_the_restatement(tile, dtype):
    crossed = 0
    for off, col, val, x in small_merge_matrices(dtype):
        got = oracle.spmv_merge(off, col, val, x, tile_items=tile)
        ref = merge_restated(off, col, val, x, tile)
        u = np.uint32 if dtype == F32 else np.uint64
        bad = np.flatnonzero(got.view(u) != ref.view(u))
        assert same(got, ref), (tile, bad[:5], got[bad[:5]], ref[bad[:5]])
        crossed = max(crossed, int(kf.merge_crossings(off, tile).max()))
    assert crossed >= (2 if tile <= 1024 else 1)  # (a row with several carries was among them)


# ---- every case of the device tests: the models against the reference, and what they can tell apart ---------------------------
def changed(a, b):
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return int((a.view(u) != b.view(u)).sum())


def lane_blind(variant, lanes, other, off, dtype, tail):
    """why a case cannot tell a wrong variant of the lane-group order from the right one (None: it can)"""
    s, e = off[:-1].astype(np.int64), off[1:].astype(np.int64)
    if tail is not None:
        s, e = np.minimum(s, tail), np.minimum(e, tail)
    lo, end = np.where(e > s, s % 4, 0), np.where(e > s, e - (s & ~3), 0)  # per row: its first slot and the one behind its last
    per_lane = 2 if dtype == F64 else 4                    # contiguous slots of a lane at the start of a pass
    if variant == "row_grid":
        if lanes == 1:
            return "one lane takes every slot in ascending order wherever the grid lies"
        if not ((s % 4 != 0) & (e > s)).any():
            return "every row starts on the grid"
    if variant == "layout" and lanes == 1:
        return "one lane takes every slot in ascending order in either layout"
    if variant == "butterfly" and lanes <= 2:
        return "a butterfly of at most one step"
    if variant == "lanes":
        # With w = min(L, L') lanes a row's slots from per_lane * w on wrap round to the lanes' second pieces; with 2 w lanes they
        # are the first pieces of the lanes w, w + 1, ..., which the butterfly's step w adds to the lanes 0, 1, ...: the same bits
        # where nothing wraps, or (f64, rows that start at slot 2 or 3) where the first pieces of the lanes wrapped onto lie wholly
        # in front of the row, so that those lanes hold +0 in the one and nothing else in the other.
        w = min(lanes, other)
        wraps = end > per_lane * w
        onto = (end - 1 - per_lane * w) // per_lane        # the last lane wrapped onto
        harmless = (end <= 2 * per_lane * w) & (per_lane * onto + per_lane - 1 < lo)
        if not (wraps & ~harmless).any():
            return "no row wraps round min(L, L') lanes onto a lane that already holds entries of it"
    return None


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_lane_model_on_the_device_cases(dtype):
    told = {}
    for name, lanes, (n_cols, off, col, val, x), tail in kf.lane_cases(dtype):
        y = oracle.spmv_lanes(off, col, val, x, lanes, tail_from=tail)
        assert_spmv_close(y, off, col, val, x, "lane model, %s, lanes %d" % (name, lanes))
        variants = [(v, lanes, w) for v, w in oracle.LANES_WRONG.items()]
        variants += [("lanes", other, 0) for other in (lanes // 2, lanes * 2) if 1 <= other <= 64]
        for variant, width, wrong in variants:
            n = changed(oracle.spmv_lanes(off, col, val, x, width, tail_from=tail, wrong=wrong), y)
            why = lane_blind(variant, lanes, width, off, dtype, tail)
            assert (n == 0) if why else (n > 0), (name, lanes, variant, width, n, why)
            told[(name.split("-nnz")[0], variant)] = told.get((name.split("-nnz")[0], variant), 0) + (n > 0)
    # every variant is told apart by the ragged matrix and by the mixed-phase one at some width; the CONFIGS entries, whose rows of
    # 31 or 32 entries (7 for the stencil) are what the forms need, each tell apart what lane_blind does not excuse
    for case in ("ragged", "mixed-phases"):
        for variant in list(oracle.LANES_WRONG) + ["lanes"]:
            assert told[(case, variant)] > 0, (case, variant)


def merge_blind(variant, off):
    crossings = int(kf.merge_crossings(off).max()) if int(off[-1]) + len(off) - 1 > 2048 else 0
    if variant == "assoc" and crossings < 2:
        return "no row has two carries"
    if variant == "descending" and crossings < 3:
        return "no row has three carries (two commute)"
    if variant == "tile4096":
        # the threads' items and the waves are the same in both: only a row with entries on both sides of an odd multiple of 2048
        # items, and in more than the first thread behind it, is summed in another order
        n_rows, nnz = len(off) - 1, int(off[-1])
        d = np.arange(2048, n_rows + nnz, 4096, dtype=np.uint64)
        rows, nz = oracle.merge_path_search(off, nnz, d)
        ok = [r < n_rows and off[r] < k and off[r + 1] > k + 8 for r, k in zip(rows.tolist(), nz.tolist())]
        if not any(ok):
            return "no row goes on for more than a thread's items behind an odd tile boundary"
    return None


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_merge_model_on_the_device_cases(dtype):
    told = set()
    builders = {name: b for name, (b, _) in kf.MERGE_CASES.items()}
    builders["config-merge"] = lambda dt: kf.config_matrix("merge", dt)[:4]
    for name, build in builders.items():
        n_cols, off, col, val = build(dtype)
        x = kf.vector_x(n_cols, dtype)
        y = oracle.spmv_merge(off, col, val, x)
        assert_spmv_close(y, off, col, val, x, "merge model, " + name)
        if name in kf.MERGE_CASES:
            assert int(kf.merge_crossings(off).max()) >= kf.MERGE_CASES[name][1], name
        for variant, tile, wrong in [(v, 2048, w) for v, w in oracle.MERGE_WRONG.items()] + [("tile4096", 4096, 0)]:
            n = changed(oracle.spmv_merge(off, col, val, x, tile_items=tile, wrong=wrong), y)
            why = merge_blind(variant, off)
            assert (n == 0) if why else (n > 0), (name, variant, n, why)
            if n:
                told.add(variant)
    assert told == set(oracle.MERGE_WRONG) | {"tile4096"}


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_k1_and_k1r_with_its_tail_differ_only_in_the_rows_that_hold_the_tail(dtype):
    """what tests/test_spmv_order_gpu.py and DESIGN.md section 4 say of borrowed, unpadded arrays: on the ragged matrix only the
    last row (the one with entries from nnz & ~3 on) can differ between the two orders, it does differ there at some widths (so the device test's two
    models are two), and never with one lane (the tail is then the lane's own order)"""
    seen = 0
    for mod in (1, 2, 3):
        n_cols, off, col, val = kf.ragged(dtype, mod)
        x = kf.vector_x(n_cols, dtype)
        limit = int(off[-1]) & ~3
        holders = set(np.flatnonzero(off[1:] > limit).tolist())
        assert holders == {kf.RAGGED_ROWS - 1}
        differing = set()
        for lanes in kf.LANES:
            a, b = oracle.spmv_lanes(off, col, val, x, lanes), oracle.spmv_lanes(off, col, val, x, lanes, tail_from=limit)
            rows = {int(r) for r in np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))}
            assert rows <= holders and (lanes > 1 or not rows), (mod, lanes, rows)
            differing |= rows
        seen += differing == holders
    assert seen >= 2
