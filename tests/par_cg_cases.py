"""The systems, splits and settings of tests/test_par_cg_bits_gpu.py -- test infrastructure, not product code.  They live here,
apart from the GPU file, so that tests/test_par_cg_model.py can show WITHOUT a GPU that each of them tells the right summation
order from the wrong ones (par_cg_model.WRONG): a case whose bits do not move under a mistake cannot catch it on the device.

A Case is everything the model needs: the matrix, b, x0, the cuts, tol, iter_max and whether every block's p.Ap is fused.  The
seeds were chosen by that CPU test's own rule: raise the seed from 0 until every applicable mistake moves a bit."""
import functools
import math

import numpy as np

import cg_model
import par_cg_model

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
IDS = ["f32", "f64"]

# 1, 2, 3, 5, 255, 257: one workgroup; every tail length, fewer rows than lanes, a second 256-row tile.  2051: a second workgroup
# in launch_dot and in the update sweep.  The block starts 0, 1, 3, 6, 11, 266, 523 take every residue mod 4 (f32) and mod 2 (f64).
HEIGHTS = [1, 2, 3, 5, 255, 257, 2051]
SPLIT7 = [0] + np.cumsum(HEIGHTS).tolist()              # [0, 1, 3, 6, 11, 266, 523, 2574]
SPLIT7_REV = [0] + np.cumsum(HEIGHTS[::-1]).tolist()    # the big block first: it starts aligned
N7 = SPLIT7[-1]
BODIES = 6

EVEN_N = 3 * 1024 + 5                                    # with_sub_matrices(3, ...): R = 1025, the last block 1027 rows
EVEN_CUTS = [0, 1025, 2050, EVEN_N]
GATHER_N = 3077
GATHER_CUTS = [0, 1025, 2050, GATHER_N]
# block 0: 1 048 576 + 2051 rows: reduce_blocks = 514 > the update sweep's 512 workgroups, 514 in launch_dot; block 1: 524 288 + 1027
# rows = 2053 tiles of 256: reduce_blocks(tiles) = 2 workgroups in launch_fold2; block 2: 5 rows.  The smallest heights that do.
CAPS_CUTS = [0, 1_048_576 + 2051, 1_048_576 + 2051 + 524_288 + 1027, 1_048_576 + 2051 + 524_288 + 1027 + 5]
AUTO_N, AUTO_K, AUTO_BLOCKS, AUTO_BODIES = 40_000, 32, 4, 5
AUTO_CUTS = [k * (AUTO_N // AUTO_BLOCKS) for k in range(AUTO_BLOCKS + 1)]
EMPTY_CUTS = [0, 259, 259, 1030]                         # block 1 has no row; block 2 starts unaligned in both types


def rhs(n, dtype, seed, x0_random):
    rng = np.random.default_rng(1000 + seed)
    b = rng.uniform(-1, 1, n).astype(dtype)
    x_rand = rng.uniform(-1, 1, n).astype(dtype)
    return b, (x_rand if x0_random else np.zeros(n, dtype))


def coupled(n, dtype, seed):
    """cg_model.tridiag plus the symmetric coupling (i, n - 1 - i) = -0.25 for i != n - 1 - i, 0.25 more on those rows' diagonal
    (still strictly diagonally dominant: SPD); columns ascending.  Every block references columns of every other: all-gather."""
    off, col, val = cg_model.tridiag(n, np.float64, seed=seed)
    rows = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    col = col.astype(np.int64)
    i = np.arange(n)
    i = i[i != n - 1 - i]
    assert (np.abs(n - 1 - 2 * i) > 1).all()             # (the partner is no tridiagonal neighbour: no duplicate position)
    val = val + 0.25 * ((rows == col) & (rows != n - 1 - rows))
    rows, col, val = np.concatenate([rows, i]), np.concatenate([col, n - 1 - i]), np.concatenate([val, np.full(len(i), -0.25)])
    order = np.lexsort((col, rows))
    out = np.zeros(n + 1, np.uint32)
    np.cumsum(np.bincount(rows, minlength=n), out=out[1:])
    return out, col[order].astype(np.uint32), val[order].astype(dtype)


class Case:
    def __init__(self, name, dtype, parts, b, x0, cuts, tol=0.0, iter_max=BODIES, fused=False):
        self.name, self.dtype, self.parts, self.b, self.x0 = name, dtype, parts, b, x0
        self.cuts, self.tol, self.iter_max, self.fused = list(cuts), tol, iter_max, fused
        self.n = len(parts[0]) - 1

    def model(self, wrong=(), product=None, **over):
        kw = dict(tol=self.tol, iter_max=self.iter_max)
        kw.update(over)
        return par_cg_model.par_cg(*self.parts, self.b, self.x0, kw["tol"], kw["iter_max"], self.cuts, fused=self.fused, product=product, wrong=wrong)

    def with_(self, **kw):
        c = Case(self.name, self.dtype, self.parts, self.b, self.x0, self.cuts, self.tol, self.iter_max, self.fused)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def blocks(self):
        """(rows, n, off, col, val) of every block: its rows of the global matrix, global columns"""
        off, col, val = self.parts
        out = []
        for r0, r1 in zip(self.cuts[:-1], self.cuts[1:]):
            o = off[r0:r1 + 1].astype(np.int64)
            out.append((r1 - r0, self.n, (o - o[0]).astype(np.uint32), col[o[0]:o[-1]], val[o[0]:o[-1]]))
        return out


# The seed of every case, by (case name, dtype name): the smallest from 0 at which every applicable mistake moves a bit of what
# the device reports (tests/test_par_cg_model.py::test_gpu_cases_tell_right_from_wrong checks exactly that; a case not listed: 0).
# The two caps cases share one matrix, hence one seed ("caps"): the smallest that serves both.
SEEDS = {
    ("split7-separate-x0", "float32"): 1,
    ("split7-rev-separate-zero", "float32"): 8,
    ("split7-rev-separate-x0", "float32"): 17,
    ("stop-separate", "float32"): 1,
    ("iter_max-5", "float32"): 1,
    ("iter_max-2", "float32"): 2,
    ("split7-separate-x0", "float64"): 2,
    ("split7-rev-separate-zero", "float64"): 15,
    ("split7-rev-separate-x0", "float64"): 4,
    ("split7-rev-fused-zero", "float64"): 1,
    ("even3-separate", "float64"): 1,
    ("gather3-separate", "float64"): 2,
    ("stop-separate", "float64"): 2,
    ("iter_max-5", "float64"): 2,
    ("iter_max-2", "float64"): 2,
    ("caps", "float32"): 4,
    ("caps", "float64"): 4,
}


def seed_of(name, dtype):
    return SEEDS.get((name, np.dtype(dtype).name), 0)


def tag(fused):
    return "fused" if fused else "separate"


@functools.lru_cache(maxsize=None)
def split7(dtype, reverse, fused, x0_random, seed=None):
    name = "split7%s-%s-%s" % ("-rev" if reverse else "", tag(fused), "x0" if x0_random else "zero")
    seed = seed_of(name, dtype) if seed is None else seed
    b, x0 = rhs(N7, dtype, seed, x0_random)
    return Case(name, dtype, cg_model.tridiag(N7, dtype, seed=seed), b, x0, SPLIT7_REV if reverse else SPLIT7, fused=fused)


@functools.lru_cache(maxsize=None)
def even3(dtype, fused, seed=None):
    name = "even3-" + tag(fused)
    seed = seed_of(name, dtype) if seed is None else seed
    b, x0 = rhs(EVEN_N, dtype, seed, True)
    return Case(name, dtype, cg_model.tridiag(EVEN_N, dtype, seed=seed), b, x0, EVEN_CUTS, fused=fused)


@functools.lru_cache(maxsize=None)
def gather3(dtype, fused, seed=None):
    name = "gather3-" + tag(fused)
    seed = seed_of(name, dtype) if seed is None else seed
    b, x0 = rhs(GATHER_N, dtype, seed, True)
    return Case(name, dtype, coupled(GATHER_N, dtype, seed), b, x0, GATHER_CUTS, fused=fused)


@functools.lru_cache(maxsize=2)
def caps_system(dtype, seed):
    n = CAPS_CUTS[-1]
    return cg_model.tridiag(n, dtype, seed=seed), rhs(n, dtype, seed, True)


def caps(dtype, fused, seed=None):
    parts, (b, x0) = caps_system(dtype, seed_of("caps", dtype) if seed is None else seed)   # (one matrix for both variants)
    return Case("caps-" + tag(fused), dtype, parts, b, x0, CAPS_CUTS, iter_max=3, fused=fused)


STOP_BODY = 4


@functools.lru_cache(maxsize=None)
def stop_case(dtype, fused, seed=None):
    """The 7-block split with a tol strictly between sqrt(rr_4) and the smallest earlier sqrt(rr): the loop has to leave in body
    4, neither sooner nor later, whatever the batching."""
    name = "stop-" + tag(fused)
    seed = seed_of(name, dtype) if seed is None else seed
    b, x0 = rhs(N7, dtype, seed, True)
    base = Case(name, dtype, cg_model.tridiag(N7, dtype, seed=seed), b, x0, SPLIT7, fused=fused, iter_max=8)
    norms = [math.sqrt(float(v)) for v in base.model().rr_list]
    lo, hi = norms[STOP_BODY - 1], min(norms[:STOP_BODY - 1])
    assert lo < 0.9 * hi, norms  # (the gap the test needs; far wider than any rounding of the square root)
    return base.with_(tol=0.5 * (lo + hi), iter_max=50)


@functools.lru_cache(maxsize=None)
def limits_case(dtype, iter_max, seed=None):
    name = "iter_max-%d" % iter_max
    seed = seed_of(name, dtype) if seed is None else seed
    b, x0 = rhs(N7, dtype, seed, True)
    return Case(name, dtype, cg_model.tridiag(N7, dtype, seed=seed), b, x0, SPLIT7, iter_max=iter_max)


@functools.lru_cache(maxsize=None)
def empty_block(dtype, fused, seed=None):
    name = "empty-" + tag(fused)
    seed = seed_of(name, dtype) if seed is None else seed
    n = EMPTY_CUTS[-1]
    b, x0 = rhs(n, dtype, seed, True)
    return Case(name, dtype, cg_model.tridiag(n, dtype, seed=seed), b, x0, EMPTY_CUTS, fused=fused)


@functools.lru_cache(maxsize=None)
def auto_blocks(dtype=F32, seed=None):
    """test_adopted_device_born_blocks' matrix (banded-stratified, 40 000 x 32, f32, 4 blocks of 10 000 rows: AUTO = the ring
    kernel per block, p.Ap by the separate dot).  Not symmetric: the recurrence is defined all the same."""
    import oracle
    from sparsemat_amd import synth
    assert dtype == F32
    parts = oracle.gen_fixed(synth.SEED_MATRIX, synth.PATTERN_BANDED, AUTO_N, AUTO_K, F32)
    b, x0 = rhs(AUTO_N, F32, seed_of("auto-blocks", F32) if seed is None else seed, True)
    return Case("auto-blocks", F32, parts, b, x0, AUTO_CUTS, iter_max=AUTO_BODIES)


def builders(dtype):
    """every case of the GPU file for one value type: [(name, builder(seed=None) -> Case)]"""
    out = [("split7%s-%s-%s" % ("-rev" if rev else "", tag(fused), "x0" if x0r else "zero"), functools.partial(split7, dtype, rev, fused, x0r))
           for rev in (False, True) for fused in (False, True) for x0r in (False, True)]
    for fam, what in ((even3, "even3"), (gather3, "gather3"), (caps, "caps"), (stop_case, "stop"), (empty_block, "empty")):
        out += [("%s-%s" % (what, tag(fused)), functools.partial(fam, dtype, fused)) for fused in (False, True)]
    out += [("iter_max-%d" % it, functools.partial(limits_case, dtype, it)) for it in (5, 2, 0)]
    if dtype == F32:
        out.append(("auto-blocks", functools.partial(auto_blocks, dtype)))
    return out


def applicable(case, wrong):
    """Can this mistake move a bit of what the device reports (x, every r.r, the body count) in this case at all?"""
    heights = np.diff(case.cuts)
    live = int((heights > 0).sum())
    if wrong == "aligned":     # (a separate dot from an unaligned block start)
        return case.iter_max > 0 and not case.fused and any(h > 0 and not par_cg_model.block_start_aligned(r0, case.dtype) for r0, h in zip(case.cuts, heights))
    if wrong == "single_fold":
        return case.iter_max > 0 and case.fused and live >= 2
    if wrong == "order":       # (two values: a + b == b + a, and a +0 beside them changes nothing; three: the tree adds (v0 + v2) + v1)
        return live >= 3
    if wrong == "drop_last":
        return heights[-1] > 0
    if wrong == "late_stop":   # (shows in p alone, which no entry point returns: tests/test_par_cg_model.py looks at p)
        return False
    assert wrong == "stop_next"
    return case.tol > 0.0


def observable(res):
    """what the device hands back: x, the r.r of every body (the last one is reported; the earlier ones decide the stop and feed
    beta), the initial r.r (reported when no body runs) and the body count"""
    return res.x, np.array([res.rr0] + list(res.rr_list)), res.iterations


def same(a, b):
    """bit equality (any NaN equals any NaN: its sign and payload are not arithmetic)"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def differs(a, b):
    """does any bit of what the device reports differ?"""
    (xa, ra, ia), (xb, rb, ib) = observable(a), observable(b)
    return ia != ib or not (same(xa, xb) and same(ra, rb))
