"""The job table of the threading test (tests/thread_child.py runs it, tests/test_threads_gpu.py starts that program,
tests/test_thread_jobs_host.py checks the table itself on the CPU).  Importing this module touches no device.

A job is run(inp, sm) -> [(label, bytes)]: it creates its own handles and vectors from the read-only host arrays of `inp`
(build_inputs(), called once on the main thread before any thread starts), makes a fixed sequence of calls, returns the bytes of
what came back together with the integers it read (iterations, routes, getters, the bytes of prepare_stats), and drops everything
it made.  A job with a `verify` is held, in the serial pass of the child, to a reference outside the library -- the same call the
operation's own GPU test makes.  No job reads or writes os.environ: the library reads its knobs lazily with getenv, so only
those entries of kernel_forms.CONFIGS qualify whose `env` asks for nothing but unset variables, and the child runs without any
SMH_* variable.

The shapes are the ones the suite has established: the matrices of kernel_forms.CONFIGS, laplace24 and stencil7(24^3) for the
solvers (tol = 0, iter_max = 11, check_every = 4), hex_stream(24) of test_crs_update_gpu.py, the "band" and "repeat" shapes of
test_transpose_gpu.py, the red-black 64 x 65 grid of test_sgs_gpu.py.

Graph capture: a solve captures and replays its batch only while its thread is the only one the library counts (csrc/internal.hpp,
"host threads and graph capture").  That holds in the serial pass.  In the threaded passes it never does -- all T workers are
counted in status_calls() before the first job -- so there every body is launched one by one (the same bits), and capture and
replay beside other threads are NOT exercised by the table.  What is: a thread that arrives while a lone thread captures
(thread_child.handshake)."""
import contextlib
import hashlib
import io
import math

import numpy as np

import oracle
from kernel_forms import CONFIGS, F32, F64, same, stencil7, vector_x

T = 8                      # threads of the child
ITER_MAX, CHECK_EVERY, RESTART = 11, 4, 4
PRODUCT_CONFIGS = ("k1-lanes8", "k1r-col12-auto", "k1r-banded", "merge", "colblock", "colfused", "colsplit", "tiled", "k1s-xdv", "k1s-plain",
                   "auto-arrowhead")
SOLVER_MATRICES = {"laplace24": F32, "stencil7": F64}    # (one value type each: the table is run sixteen times over)
SOLVER_VARIANTS = ("stream", "seq")                      # both the oracle's product bit for bit
VEC_SIZES = (1, 255, 4097, 100_003)
NAME = {np.dtype(F32): "f32", np.dtype(F64): "f64"}


def qualifies(cfg):
    """no environment knob to set: every value of env is None (the variable is unset, as in the child's environment)"""
    return all(v is None for v in cfg.env.values())


def i64(*v):
    return np.array(v, np.int64).tobytes()


def f64(*v):
    return np.array(v, np.float64).tobytes()


def crs_bytes(h):
    """[(label, bytes)] of a handle: its dimensions and orphan count, then its three arrays"""
    off, col, val = h.raw_parts()
    return [("dims", i64(h.n_rows(), h.n_cols(), h.n_non_zero_entries(), h.orphans())), ("off", off.tobytes()), ("col", col.tobytes()),
            ("val", val.tobytes())]


def prefixed(prefix, items):
    return [(prefix + "/" + k, v) for k, v in items]


class Got:
    """the results of one job by label, decoded"""

    def __init__(self, results):
        self.d = dict(results)
        assert len(self.d) == len(results), "a label twice"

    def arr(self, label, dtype):
        return np.frombuffer(self.d[label], dtype)

    def ints(self, label):
        return tuple(int(v) for v in np.frombuffer(self.d[label], np.int64))

    def text(self, label):
        return self.d[label].decode()

    def crs(self, prefix, dtype):
        """(n_rows, n_cols, off, col, val, orphans): the tuple the models of the builders speak"""
        n_rows, n_cols, _, orph = self.ints(prefix + "/dims")
        return n_rows, n_cols, self.arr(prefix + "/off", np.uint32), self.arr(prefix + "/col", np.uint32), self.arr(prefix + "/val", dtype), orph


def assert_crs(got, want, what):
    """got: Got.crs(); want: (n_rows, n_cols, off, col, val[, orphans or stored]) -- dimensions, offsets and columns equal, values bit
    for bit"""
    n_rows = want[0]
    assert got[:2] == tuple(want[:2]), (what, "dimensions", got[:2], want[:2])
    assert np.array_equal(got[2], np.asarray(want[2], np.uint32)[:n_rows + 1] if n_rows else np.zeros(1, np.uint32)), (what, "offsets")
    assert np.array_equal(got[3], want[3]), (what, "columns")
    assert got[4].dtype == want[4].dtype and got[4].tobytes() == np.ascontiguousarray(want[4]).tobytes(), (what, "values")


# ---- the host arrays ---------------------------------------------------------------------------------------------------------
def band_crs(rng, n_rows, n_cols, slope, below, above, max_len, dtype, shuffle):
    """tests/test_transpose_gpu.py's generator: rows with up to max_len distinct columns from [slope r - below, slope r + above]"""
    lens = rng.integers(0, max_len + 1, n_rows)
    cols, off = [], np.zeros(n_rows + 1, np.uint32)
    for r in range(n_rows):
        c0, c1 = max(0, int(slope * r) - below), min(n_cols, int(slope * r) + above + 1)
        k = min(int(lens[r]), max(0, c1 - c0))
        c = np.sort(rng.choice(np.arange(c0, c1), k, replace=False)) if k else np.zeros(0, np.int64)
        if shuffle:
            rng.shuffle(c)
        cols.append(c)
        off[r + 1] = off[r] + k
    col = np.concatenate(cols).astype(np.uint32)
    return off, col, rng.uniform(-1, 1, len(col)).astype(dtype)


def transpose_shape(shape, dtype):
    """"band" (takes the bucketed route) and "repeat" (one pair twice: the general route) of test_transpose_gpu.py"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(shape.encode()))
    off, col, val = band_crs(rng, 5000, 5100, 1.0, 40, 60, 24, dtype, shape != "band")
    if shape == "repeat":
        r = 2500
        while off[r + 1] - off[r] < 2:
            r += 1
        col[off[r] + 1] = col[off[r]]
    if col[1] < col[0]:
        col[0], col[1] = col[1], col[0]
    return 5000, 5100, off, col, val


def hex_stream(g, dtype, rng):
    """tests/test_crs_update_gpu.py's element stream: the 64 pairs of the 8 corners of every cell of a g^3 grid"""
    nodes = np.arange((g + 1) ** 3, dtype=np.uint32).reshape(g + 1, g + 1, g + 1)
    corners = np.stack([nodes[dx:g + dx, dy:g + dy, dz:g + dz].ravel() for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)], axis=1)
    rows = np.repeat(corners, 8, axis=1).ravel()
    cols = np.tile(corners, (1, 8)).ravel()
    return rows, cols, rng.uniform(-1, 1, len(rows)).astype(dtype)


def rand_crs(rng, n_rows, n_cols, max_len, dtype):
    """tests/test_crs_add_gpu.py's rand: rows of 0 .. max_len entries, columns in draw order"""
    lens = rng.integers(0, max_len + 1, n_rows)
    off = np.zeros(n_rows + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    col = rng.integers(0, n_cols, int(off[-1])).astype(np.uint32)
    return n_rows, n_cols, off, col, rng.uniform(-1, 1, len(col)).astype(dtype)


def build_inputs():
    """name -> tuple of read-only arrays (and plain integers).  Main thread only: the pattern builders of kernel_forms.py are
    lru_cache'd."""
    import sgs_model
    inp = {}
    for name in PRODUCT_CONFIGS:
        cfg = CONFIGS[name]
        assert qualifies(cfg), name
        for dtype in cfg.dtypes:                                          # (both value types where the entry has both)
            off, col, val = cfg.build(dtype)
            n = len(off) - 1
            inp["cfg/%s/%s" % (name, NAME[np.dtype(dtype)])] = (n, off, col, val) + tuple(vector_x(n, dtype, seed) for seed in (7, 8, 9))
    for name, dtype in SOLVER_MATRICES.items():
        off, col, val = oracle.laplace3d(24, 24, 24, dtype) if name == "laplace24" else stencil7((24, 24, 24), dtype)
        n = len(off) - 1
        rng = np.random.default_rng(1000 + n)
        b, x0 = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
        B, X0 = rng.uniform(-1, 1, (3, n)).astype(dtype), rng.uniform(-1, 1, (3, n)).astype(dtype)
        inp["sys/" + name] = (n, off, col, val, b, x0, B, X0)
    rng = np.random.default_rng(3)
    inp["hex24"] = hex_stream(24, F32, rng)
    for shape in ("band", "repeat"):
        inp["transpose/" + shape] = transpose_shape(shape, F64 if shape == "band" else F32)
    rng = np.random.default_rng(31)
    a = rand_crs(rng, 500, 300, 7, F32)
    b = rand_crs(rng, 500, 300, 7, F32)
    inp["rand/a"], inp["rand/b"], inp["rand/bt"] = a, b, rand_crs(rng, 300, 500, 5, F32)
    rows_a = np.repeat(np.arange(500, dtype=np.uint32), np.diff(a[2].astype(np.int64)))
    k = rng.permutation(len(rows_a))[:1500]
    inp["ops/existing"] = (rows_a[k], a[3][k], rng.uniform(-1, 1, len(k)).astype(F32), (rng.random(len(k)) < 0.1).astype(np.uint8))
    inp["ops/new"] = (rng.integers(0, 520, 3000).astype(np.uint32), rng.integers(0, 320, 3000).astype(np.uint32),
                      rng.uniform(-1, 1, 3000).astype(F32), (rng.random(3000) < 0.1).astype(np.uint8))
    inp["ops/values2"] = (rng.uniform(-1, 1, len(k)).astype(F32),)
    inp["get"] = (rng.integers(0, 520, 2000).astype(np.uint32), rng.integers(0, 320, 2000).astype(np.uint32))
    off, col, val = sgs_model.lap2d(64, 65, F64, seed=2, spread=1.0)
    n = len(off) - 1
    inp["grid"] = (n, off, col, val, rng.uniform(-1, 1, n).astype(F64), (val * np.float64(1.25)).astype(F64))
    for dtype in (F32, F64):
        for n in VEC_SIZES:
            r = np.random.default_rng(n + 1)
            inp["vec/%s/%d" % (NAME[np.dtype(dtype)], n)] = (r.uniform(-2, 2, n).astype(dtype), r.uniform(-2, 2, n).astype(dtype))
        r = np.random.default_rng(2051 + 5)
        inp["mvec/" + NAME[np.dtype(dtype)]] = (r.uniform(-1, 1, (3, 2051)).astype(dtype), r.uniform(-1, 1, (3, 2051)).astype(dtype))
    for v in inp.values():
        for a in v:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return inp


def input_digests(inp):
    out = {}
    for name, v in sorted(inp.items()):
        h = hashlib.sha256()
        for a in v:
            h.update(a.tobytes() if isinstance(a, np.ndarray) else repr(a).encode())
        out[name] = h.hexdigest()
    return out


# ---- the jobs ----------------------------------------------------------------------------------------------------------------
class Job:
    def __init__(self, name, family, run, verify=None):
        self.name, self.family, self.run, self.verify = name, family, run, verify


def quiet(fn, *args):
    """util.assert_spmv_close prints one line of bucket statistics per call: not wanted sixty times in the child's output"""
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args)


def product_job(name, dtn):
    cfg = CONFIGS[name]
    key = "cfg/%s/%s" % (name, dtn)

    def run(inp, sm):
        n, off, col, val, *xs = inp[key]
        a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
        cfg.knobs(a)
        a.prepare(cfg.variant)
        cfg.check(a)
        out = [("y%d" % k, a.mvp(x, variant=cfg.variant).tobytes()) for k, x in enumerate(xs)]
        out.append(("inner_prod", f64(a.inner_prod(xs[0][:n], xs[1], variant=cfg.variant))))
        cfg.check(a)
        family, lanes = a.resolved_variant()
        out.append(("resolved_variant", ("%s/%d" % (family, lanes)).encode()))
        out.append(("prepare_bytes", i64(a.prepare_stats(cfg.variant)[1])))
        return out

    def verify(inp, got, sm):
        from util import assert_spmv_close
        n, off, col, val, *xs = inp[key]
        for k, x in enumerate(xs):
            y = got.arr("y%d" % k, val.dtype)
            quiet(assert_spmv_close, y, off, col, val, x, "%s %s x%d" % (name, dtn, k))
            if cfg.variant in ("seq", "stream"):
                assert same(y, oracle.spmv(off, col, val, x)), (name, dtn, k, "K1s is not the oracle's product bit for bit")
        assert got.ints("prepare_bytes")[0] >= 0

    return Job("product/%s/%s" % (name, dtn), "products", run, verify)


# -- solvers
def _entries(sm, make, a, b, x0, vec=True, **kw):
    """[(entry point, solver, x)]: the DenseVec entry point with check_every = CHECK_EVERY, then the host one"""
    out = []
    if vec:
        s = make(check_every=CHECK_EVERY)
        bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x0)
        s.solve(a, bd, xd, **kw)
        assert same(bd.to_numpy(), b)
        out.append(("vec", s, xd.to_numpy()))
    s = make()
    x = x0.copy()
    s.solve(a, b, x, **kw)
    out.append(("host", s, x))
    return out


SOLVERS = ("cg", "pcg", "sgs", "ilu", "fsai", "bicgstab", "gmres", "gmres-ilu", "bicgstab-ilu")


def solver_job(kind, mat, variant):
    def run(inp, sm):
        n, off, col, val, b, x0 = inp["sys/" + mat][:6]
        a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
        out, kw, extra = [], {}, ()
        if kind == "sgs":
            perm, stats = a.color()
            out += [("perm", perm.tobytes()), ("n_colors", i64(stats["n_colors"], stats["n_rounds"]))]
            a = a.permute_symmetric(perm)
            out += prefixed("permuted", crs_bytes(a))
        a.prepare(variant)
        common = dict(tol=0.0, iter_max=ITER_MAX, variant=variant)
        if kind.endswith("ilu"):
            f, zp = a.ilu0()
            out += [("factor", f.raw_parts()[2].tobytes()), ("zero_pivot", i64(-1 if zp is None else zp))]
            kw = dict(factor=f)
        if kind == "fsai":
            g, gt, bad = a.fsai()
            out += prefixed("g", crs_bytes(g)) + prefixed("gt", crs_bytes(gt)) + [("not_spd", i64(-1 if bad is None else bad))]
            kw = dict(factor=(g, gt))
        if kind == "cg":
            runs = _entries(sm, lambda **c: sm.ConjugateGradient(0.0, ITER_MAX, variant, **c), a, b, x0)
        elif kind == "pcg":
            runs = _entries(sm, lambda **c: sm.JacobiConjugateGradient(**common), a, b, x0, vec=False)
        elif kind == "sgs":
            runs = _entries(sm, lambda **c: sm.SGSConjugateGradient(**common, **c), a, b, x0)
        elif kind == "ilu":
            runs = _entries(sm, lambda **c: sm.ILUConjugateGradient(**common, **c), a, b, x0, **kw)
        elif kind == "fsai":
            runs = _entries(sm, lambda **c: sm.FSAIConjugateGradient(**common, **c), a, b, x0, **kw)
        elif kind.startswith("bicgstab"):
            runs = _entries(sm, lambda **c: sm.BiCGStab(**common, precond="ilu" if kw else None, **c), a, b, x0, **kw)
            extra = ("breakdown",)
        else:
            runs = _entries(sm, lambda **c: sm.GMRES(**common, restart=RESTART, precond="ilu" if kw else None, **c), a, b, x0, **kw)
            extra = ("cycles", "breakdown")
        for entry, s, x in runs:
            out += [(entry + "/x", x.tobytes()), (entry + "/iterations", i64(s.iterations)), (entry + "/rr", f64(s.r_norm_squared))]
            out += [(entry + "/" + e, i64(getattr(s, e))) for e in extra]
        return out

    def verify(inp, got, sm):
        import bicgstab_model as bm
        import cg_model
        import color_model
        import fsai_model as fm
        import gmres_model as gm
        import ilu_model as im
        import pbicgstab_model as pb
        import pgmres_model as pm
        import reorder_model as rm
        import sgs_model as sg
        from util import assert_spmv_close
        n, off, col, val, b, x0 = inp["sys/" + mat][:6]
        dtype = val.dtype
        fused = variant == "stream"      # CG and the PCGs take p.Ap from the K1s epilogue (test_sgs_gpu.py's is_fused)
        if kind == "sgs":
            want = color_model.jones_plassmann(n, off, col, seed=0)
            assert np.array_equal(got.arr("perm", np.uint32), want["perm"]) and got.ints("n_colors") == (want["n_colors"], want["n_rounds"])
            off, col, val = rm.permute_symmetric(n, off, col, val, want["perm"])
            assert_crs(got.crs("permuted", dtype), (n, n, off, col, val), "permute_symmetric")
        precond = None
        if kind.endswith("ilu"):
            w, zp = _cached(("ilu", mat), lambda: im.ilu0(off, col, val, vector=True))
            assert same(got.arr("factor", dtype), w) and got.ints("zero_pivot")[0] == (-1 if zp is None else zp)
            precond = pm.ilu(off, col, w)
        if kind == "fsai":
            goff, gcol, gval, bad = _cached(("fsai", mat), lambda: fm.fsai(off, col, val))
            gp, gtp = (goff, gcol, gval), fm.transpose(goff, gcol, gval)
            assert bad is None and got.ints("not_spd")[0] == -1
            assert_crs(got.crs("g", dtype), (n, n) + gp, "g")
            assert_crs(got.crs("gt", dtype), (n, n) + tuple(gtp), "gt")
            # z = G^T (G r) by the device's own AUTO products of g and gt, each held to the parity bound (test_fsai_gpu.py's checked_apply)
            handles = [sm.SparseMatCRS.from_raw_parts(n, n, *p) for p in (gp, gtp)]

            def checked(h, parts):
                def product(v):
                    y = h.mvp(np.ascontiguousarray(v, dtype), variant="auto")
                    quiet(assert_spmv_close, y, *parts, np.ascontiguousarray(v, dtype), "fsai factor product")
                    return y
                return product
            first, second = checked(handles[0], gp), checked(handles[1], gtp)
            precond = lambda r: second(first(r))
        if kind == "cg":
            want = cg_model.cg(off, col, val, b, x0, 0.0, ITER_MAX, fused=fused)
        elif kind == "pcg":
            want = cg_model.pcg(off, col, val, b, x0, 0.0, ITER_MAX, fused=fused)
        elif kind in ("sgs", "ilu", "fsai"):
            want = sg.sgs_pcg(off, col, val, b, x0, 0.0, ITER_MAX, fused=fused, precond=precond)
        elif kind == "bicgstab":
            want = bm.bicgstab(off, col, val, b, x0, 0.0, ITER_MAX)
        elif kind == "bicgstab-ilu":
            want = pb.pbicgstab(off, col, val, b, x0, 0.0, ITER_MAX, precond)
        elif kind == "gmres":
            want = gm.gmres(off, col, val, b, x0, 0.0, ITER_MAX, RESTART)
        else:
            want = pm.pgmres(off, col, val, b, x0, 0.0, ITER_MAX, RESTART, precond)
        assert want.iterations == ITER_MAX and np.isfinite(want.x).all()
        for entry in ("host",) if kind == "pcg" else ("vec", "host"):
            what = (kind, mat, variant, entry)
            x = got.arr(entry + "/x", dtype)
            assert got.ints(entry + "/iterations")[0] == want.iterations, (what, "iterations")
            assert same(got.arr(entry + "/rr", np.float64), np.float64(want.r_norm_squared)), (what, "r.r", got.arr(entry + "/rr", np.float64), want.r_norm_squared)
            if kind.startswith("bicgstab"):
                assert got.ints(entry + "/breakdown")[0] == want.breakdown, (what, "breakdown")
            if kind.startswith("gmres"):
                assert (got.ints(entry + "/cycles")[0], got.ints(entry + "/breakdown")[0]) == (want.cycles, want.breakdown), (what, "cycles, breakdown")
            bad = np.flatnonzero(x != want.x)
            assert same(x, want.x), (what, "x", len(bad), bad[:5], x[bad[:5]], want.x[bad[:5]])

    return Job("solver/%s/%s/%s" % (kind, mat, variant), "solvers", run, verify)


_CACHE = {}


def _cached(key, make):
    """a model's factor, computed once per matrix and shared by the jobs that need it (serial pass only)"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def cg_many_job(mat):
    def run(inp, sm):
        n, off, col, val = inp["sys/" + mat][:4]
        B, X0 = inp["sys/" + mat][6:8]
        a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
        s = sm.ConjugateGradient(0.0, ITER_MAX, check_every=CHECK_EVERY)
        bm_, xm = sm.MultiVec.from_vecs(np.ascontiguousarray(B)), sm.MultiVec.from_vecs(np.ascontiguousarray(X0))
        s.solve_many(a, bm_, xm)
        out = [("vec/x", xm.to_numpy().tobytes()), ("vec/iterations", i64(*s.iterations)), ("vec/rr", f64(*s.r_norm_squared))]
        s = sm.ConjugateGradient(0.0, ITER_MAX)
        x = np.array(X0, copy=True)
        s.solve_many(a, B, x)
        return out + [("host/x", x.tobytes()), ("host/iterations", i64(*s.iterations)), ("host/rr", f64(*s.r_norm_squared))]

    def verify(inp, got, sm):
        import cg_many_model
        n, off, col, val = inp["sys/" + mat][:4]
        B, X0 = inp["sys/" + mat][6:8]
        want = cg_many_model.cg_many(off, col, val, B, X0, 0.0, ITER_MAX)
        for entry in ("vec", "host"):
            assert got.ints(entry + "/iterations") == tuple(int(v) for v in want.iterations), (mat, entry)
            assert same(got.arr(entry + "/rr", np.float64), want.r_norm_squared), (mat, entry, "r.r")
            assert same(got.arr(entry + "/x", val.dtype).reshape(3, n), want.x), (mat, entry, "x")

    return Job("solver/cg_many/" + mat, "solvers", run, verify)


# -- builders
def handle(sm, m, validate=False):
    return sm.SparseMatCRS.from_raw_parts(m[0], m[1], m[2], m[3], m[4], validate=validate)


def tup(m):
    """an input matrix as the models' (n_rows, n_cols, off, col, val, orphans)"""
    return tuple(m[:5]) + (0,)


def assemble_job():
    def run(inp, sm):
        rows, cols, vals = inp["hex24"]
        return crs_bytes(sm.SparseMatCRS.from_triplets(rows, cols, vals))

    def verify(inp, got, sm):
        rows, cols, vals = inp["hex24"]
        g = Got(prefixed("m", list(got.d.items())))
        assert_crs(g.crs("m", F32), oracle.assemble(rows, cols, vals), "assembly of hex_stream(24)")

    return Job("builder/assemble", "builders", run, verify)


def transpose_job(shape):
    def run(inp, sm):
        m = handle(sm, inp["transpose/" + shape], validate=True)
        t = m.transpose()
        return [("route", sm.SparseMatCRS.last_transpose_route().encode())] + prefixed("t", crs_bytes(t))

    def verify(inp, got, sm):
        _, _, off, col, val = inp["transpose/" + shape]
        assert got.text("route") == ("bucketed" if shape == "band" else "general"), got.text("route")
        want = oracle.transpose(off, col, val)
        assert_crs(got.crs("t", val.dtype), want, "transpose " + shape)
        assert got.ints("t/dims")[2] + got.ints("t/dims")[3] == want[5]

    return Job("builder/transpose/" + shape, "builders", run, verify)


def prod_job():
    def run(inp, sm):
        return crs_bytes(handle(sm, inp["rand/a"]).prod(handle(sm, inp["rand/bt"])))

    def verify(inp, got, sm):
        g = Got(prefixed("m", list(got.d.items())))
        want = oracle.prod(inp["rand/a"], inp["rand/bt"])
        assert_crs(g.crs("m", F32), want, "prod")
        assert g.ints("m/dims")[2] + g.ints("m/dims")[3] == want[5]

    return Job("builder/prod", "builders", run, verify)


ADD_CASES = (("add", "rand/b"), ("sub", "rand/b"), ("add_assign", "rand/b"), ("add", "rand/a"), ("add_assign", "rand/a"))


def add_job():
    def run(inp, sm):
        out = []
        for k, (op, other) in enumerate(ADD_CASES):
            a, b = handle(sm, inp["rand/a"]), handle(sm, inp[other])
            if op == "add":
                r = a + b
            elif op == "sub":
                r = a - b
            else:
                a += b
                r = a
            out += [("%d/route" % k, sm.SparseMatCRS.last_add_route().encode())] + prefixed(str(k), crs_bytes(r))
        return out

    def verify(inp, got, sm):
        import add_model
        for k, (op, other) in enumerate(ADD_CASES):
            want = add_model.add(tup(inp["rand/a"]), tup(inp[other]), subtract=op == "sub")
            assert_crs(got.crs(str(k), F32), want, (op, other))
            assert got.ints("%d/dims" % k)[3] == want[5]
        assert got.text("3/route") != "general" and got.text("0/route") != got.text("3/route")   # (a + a keeps the structure)

    return Job("builder/add", "builders", run, verify)


def apply_job():
    def run(inp, sm):
        out = []
        for k, ops in enumerate(("ops/existing", "ops/new")):
            a = handle(sm, inp["rand/a"])
            a.apply(*inp[ops])
            out += [("%d/route" % k, sm.SparseMatCRS.last_apply_route().encode())] + prefixed(str(k), crs_bytes(a))
        return out

    def verify(inp, got, sm):
        import update_model
        assert (got.text("0/route"), got.text("1/route")) == ("values_only", "general")
        for k, ops in enumerate(("ops/existing", "ops/new")):
            want = update_model.apply(tup(inp["rand/a"]), *inp[ops])
            assert_crs(got.crs(str(k), F32), want, ops)
            assert got.ints("%d/dims" % k)[3] == want[5]

    return Job("builder/apply", "builders", run, verify)


def plan_job():
    def run(inp, sm):
        rows, cols, vals, ops = inp["ops/existing"]
        a = handle(sm, inp["rand/a"])
        plan = a.update_plan(rows, cols, ops)
        plan.execute(vals)
        out = prefixed("first", crs_bytes(a))
        plan.execute(inp["ops/values2"][0], from_zero=True)
        st = plan.stats()
        return out + prefixed("second", crs_bytes(a)) + [("stats", i64(st["n_ops"], st["n_targets"], st["n_live_ops"], st["longest_run"]))]

    def verify(inp, got, sm):
        import plan_model
        rows, cols, vals, ops = inp["ops/existing"]
        first = plan_model.execute(tup(inp["rand/a"]), rows, cols, vals, ops)
        assert_crs(got.crs("first", F32), first, "execute")
        assert_crs(got.crs("second", F32), plan_model.execute(first, rows, cols, inp["ops/values2"][0], ops, from_zero=True), "execute from zero")

    return Job("builder/update_plan", "builders", run, verify)


def reorder_job():
    def run(inp, sm):
        n, off, col, val = inp["grid"][:4]
        a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
        perm, st = a.rcm()
        cperm, cst = a.color()
        return ([("rcm", perm.tobytes()), ("rcm_stats", i64(st["n_components"], st["n_levels"])), ("color_perm", cperm.tobytes()),
                 ("colors", cst["colors"].tobytes()), ("color_stats", i64(cst["n_colors"], cst["n_rounds"]))]
                + prefixed("p", crs_bytes(a.permute_symmetric(perm))))

    def verify(inp, got, sm):
        import color_model
        import reorder_model as rm
        n, off, col, val = inp["grid"][:4]
        perm, comps, levels = rm.rcm(n, off, col)
        assert np.array_equal(got.arr("rcm", np.uint32), perm) and got.ints("rcm_stats") == (comps, levels)
        assert_crs(got.crs("p", val.dtype), (n, n) + tuple(rm.permute_symmetric(n, off, col, val, perm)), "permute_symmetric")
        want = color_model.jones_plassmann(n, off, col, seed=0)
        assert np.array_equal(got.arr("color_perm", np.uint32), want["perm"]) and np.array_equal(got.arr("colors", np.uint32), want["colors"])
        assert got.ints("color_stats") == (want["n_colors"], want["n_rounds"])

    return Job("builder/reorder", "builders", run, verify)


def factor_job():
    def run(inp, sm):
        n, off, col, val, r, val2 = inp["grid"]
        a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
        f, zp = a.ilu0()
        out = [("ilu", f.raw_parts()[2].tobytes()), ("zero_pivot", i64(-1 if zp is None else zp))]
        a2 = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val2)
        zp = f.ilu0_refactor(a2)
        out += [("refactor", f.raw_parts()[2].tobytes()), ("refactor_zero_pivot", i64(-1 if zp is None else zp))]
        g, gt, bad = a.fsai()
        out += prefixed("g", crs_bytes(g)) + prefixed("gt", crs_bytes(gt)) + [("not_spd", i64(-1 if bad is None else bad))]
        out += [("lower", a.trisolve(r, "lower").tobytes()), ("upper", a.trisolve(sm.DenseVec.from_vec(r), "upper").to_numpy().tobytes())]
        return out

    def verify(inp, got, sm):
        import fsai_model as fm
        import ilu_model as im
        import trisolve_model as tm
        n, off, col, val, r, val2 = inp["grid"]
        for label, v in (("ilu", val), ("refactor", val2)):
            w, zp = im.ilu0(off, col, v, vector=True)
            assert same(got.arr(label, F64), w), label
        assert got.ints("zero_pivot") == got.ints("refactor_zero_pivot") == (-1,)
        goff, gcol, gval, bad = fm.fsai(off, col, val)
        assert bad is None and got.ints("not_spd") == (-1,)
        assert_crs(got.crs("g", F64), (n, n, goff, gcol, gval), "g")
        assert_crs(got.crs("gt", F64), (n, n) + tuple(fm.transpose(goff, gcol, gval)), "gt")
        assert same(got.arr("lower", F64), tm.trisolve(off, col, val, r, tm.LOWER, False)), "trisolve lower"
        assert same(got.arr("upper", F64), tm.trisolve(off, col, val, r, tm.UPPER, False)), "trisolve upper"

    return Job("builder/factors", "builders", run, verify)


def misc_job():
    def run(inp, sm):
        a = handle(sm, inp["rand/a"])
        rows, col_ptr, entries = a.column_info()
        out = [("ci/rows", rows.tobytes()), ("ci/col_ptr", col_ptr.tobytes()), ("ci/entries", entries.tobytes()),
               ("get_many", a.get_many(*inp["get"]).tobytes())]
        c = a.clone()
        c.sort_rows()
        out += prefixed("sorted", crs_bytes(c)) + [("is_sorted", i64(c.is_sorted(), a.is_sorted()))]
        c = a.clone()
        c.scale(0.7310585786300049)
        out += prefixed("scaled", crs_bytes(c)) + prefixed("clone", crs_bytes(a.clone()))
        return out + prefixed("eye", crs_bytes(sm.SparseMatCRS.eye(1000, F64)))

    def verify(inp, got, sm):
        import update_model
        m = inp["rand/a"]
        n_rows, n_cols, off, col, val = m
        rows, col_ptr, entries = oracle.column_info(off, col, n_cols)
        assert np.array_equal(got.arr("ci/rows", np.uint32), rows) and np.array_equal(got.arr("ci/col_ptr", np.uint32), col_ptr)
        assert np.array_equal(got.arr("ci/entries", np.uint32), entries)
        assert same(got.arr("get_many", F32), update_model.get_many(tup(m), *inp["get"]))
        s = oracle.crs_sort_rows(off, col, val)
        assert_crs(got.crs("sorted", F32), (n_rows, n_cols, off, s[-2], s[-1]), "sort_rows")
        assert got.ints("is_sorted")[0] == 1
        assert_crs(got.crs("scaled", F32), (n_rows, n_cols, off, col, oracle.vec_scale(val, F32(0.7310585786300049))), "scale")
        assert_crs(got.crs("clone", F32), m, "clone")
        assert_crs(got.crs("eye", F64), update_model.eye(1000, F64), "eye")

    return Job("builder/misc", "builders", run, verify)


# -- vectors
S = 0.7310585786300049


def vec_job(dtn, n):
    dtype = F32 if dtn == "f32" else F64

    def run(inp, sm):
        a, b = inp["vec/%s/%d" % (dtn, n)]
        y = sm.DenseVec.from_vec(b)
        out = []
        for op in ("add", "axpy", "xpby", "scale"):
            x = sm.DenseVec.from_vec(a)
            if op == "add":
                x.add(y)
            elif op == "axpy":
                x.axpy(dtype(S), y)
            elif op == "xpby":
                x.xpby(dtype(S), y)
            else:
                x.scale(dtype(S))
            out.append((op, x.to_numpy().tobytes()))
        x = sm.DenseVec.from_vec(a)
        return out + [("dot", f64(x.inner_prod(y))), ("norm_squared", f64(x.norm_squared())), ("norm", f64(x.norm()))]

    def verify(inp, got, sm):
        a, b = inp["vec/%s/%d" % (dtn, n)]
        s = dtype(S)
        for op, want in (("add", oracle.vec_add(a, b)), ("axpy", oracle.vec_axpy(a, s, b)), ("xpby", oracle.vec_xpby(a, s, b)), ("scale", oracle.vec_scale(a, s))):
            assert same(got.arr(op, dtype), want), (op, dtn, n)
        # test_blas1_cg_gpu.py::test_reductions' bound on the device's fixed tree against the exact value
        eps = np.finfo(dtype).eps
        exact = float(np.dot(a.astype(np.float64), b.astype(np.float64)))
        scale = float(np.dot(np.abs(a).astype(np.float64), np.abs(b).astype(np.float64)))
        d, nn, nrm = (float(got.arr(k, np.float64)[0]) for k in ("dot", "norm_squared", "norm"))
        assert abs(d - exact) <= (np.log2(max(n, 2)) + 8) * eps * scale + 1e-300
        assert abs(nn - float(oracle.norm_squared(a))) <= 2 * max(n, 1) * eps * float(np.dot(a.astype(np.float64), a.astype(np.float64))) + 1e-300
        assert nrm == math.sqrt(nn)

    return Job("vector/%s/%d" % (dtn, n), "vectors", run, verify)


def mvec_job(dtn):
    dtype = F32 if dtn == "f32" else F64

    def run(inp, sm):
        X, Y = inp["mvec/" + dtn]
        x, y = sm.MultiVec.from_vecs(np.ascontiguousarray(X)), sm.MultiVec.from_vecs(np.ascontiguousarray(Y))
        return [("dot", f64(*x.dot(y))), ("norm_squared", f64(*x.norm_squared()))]

    def verify(inp, got, sm):
        import cg_many_model
        X, Y = inp["mvec/" + dtn]
        dot = np.array([cg_many_model.column_sum(X[c] * Y[c]) for c in range(3)], dtype)
        nsq = np.array([cg_many_model.column_sum(X[c] * X[c]) for c in range(3)], dtype)
        assert np.array_equal(got.arr("dot", np.float64), dot.astype(np.float64))
        assert np.array_equal(got.arr("norm_squared", np.float64), nsq.astype(np.float64))

    return Job("vector/multi/" + dtn, "vectors", run, verify)


def job_table():
    jobs = [product_job(name, NAME[np.dtype(dtype)]) for name in PRODUCT_CONFIGS for dtype in CONFIGS[name].dtypes]
    for mat in SOLVER_MATRICES:
        for variant in SOLVER_VARIANTS:
            jobs += [solver_job(kind, mat, variant) for kind in SOLVERS]
        jobs.append(cg_many_job(mat))
    jobs += [assemble_job(), transpose_job("band"), transpose_job("repeat"), prod_job(), add_job(), apply_job(), plan_job(), reorder_job(),
             factor_job(), misc_job()]
    jobs += [vec_job(dtn, n) for dtn in ("f32", "f64") for n in VEC_SIZES] + [mvec_job("f32"), mvec_job("f64")]
    assert len({j.name for j in jobs}) == len(jobs)
    return jobs


def rotation(t, n_jobs, n_threads=T):
    """the two passes of thread t as job indices: the table rotated by t * ceil(J / T), then the table in reverse order -- so that
    different families overlap"""
    shift = t * -(-n_jobs // n_threads)
    first = [(k + shift) % n_jobs for k in range(n_jobs)]
    return first, list(range(n_jobs - 1, -1, -1))


# ---- statuses: what a thread reads back must be its own ------------------------------------------------------------------------
def status_calls(inp, sm, t, wait):
    """Thread t makes one refused call whose message carries a number only it uses, waits (wait(): a barrier, or nothing in the
    serial pass) until every thread has made its own, and reads smh_last_error(); then the same for the three route getters, even
    threads taking one route by their matrix's shape and odd threads the other.  Returns [(label, bytes)]."""
    import ctypes as C
    n, off, col, val = inp["sys/laplace24"][:4]
    a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    x_len = 1000 + t                                    # (the largest column is 13 823: refused, a status and no fault)
    x, y = np.zeros(x_len, val.dtype), np.zeros(n, val.dtype)
    status = sm.lib().smh_crs_spmv(a._h, x.ctypes.data, x_len, y.ctypes.data, sm._lib.VARIANTS["seq"])
    wait()
    out = [("status", i64(status)), ("last_error", sm.lib().smh_last_error())]
    even = t % 2 == 0
    handle(sm, inp["transpose/band" if even else "transpose/repeat"], validate=True).transpose()
    m = handle(sm, inp["rand/a"])
    m += handle(sm, inp["rand/a" if even else "rand/b"])
    m.apply(*inp["ops/existing" if even else "ops/new"])
    wait()
    return out + [("transpose_route", sm.SparseMatCRS.last_transpose_route().encode()), ("add_route", sm.SparseMatCRS.last_add_route().encode()),
                  ("apply_route", sm.SparseMatCRS.last_apply_route().encode())]


def expected_last_error(t):
    return ("index out of bounds: the len is %d but the index is 13823" % (1000 + t)).encode()
