"""Handle lifetime: every lazily built workspace (merge table, ring plans incl. the wide and the banded ring, 16-bit
column arrays, K1s windows and codes, K2c / K2f / K2s / K2t copies, assembly scratch) is released with its handle -- also
after it was dropped and built again inside the handle's life (sort_rows, update_values, scale, another block width) -- and so is every
array the matrix operations build (transpose, prod, column_info, clone, add / sub, apply, get_many, eye, replay), every
block, stream, vector and solver workspace of a partitioned matrix (SparseMatParLocal, ParVec), and every workspace of the
single-matrix solvers (ConjugateGradient, JacobiConjugateGradient), also of a solve that fails half way -- device memory in use
returns to where it started after many create / use / destroy rounds."""
import gc
import os

import numpy as np
import pytest
import torch

import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib
from util import assert_spmv_close, random_crs

pytestmark = pytest.mark.gpu


def _used():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def _used_without_the_pool():
    import ctypes as C
    sm._lib.check(sm.lib().smh_pool_trim())
    kept, live = C.c_size_t(), C.c_size_t()
    sm._lib.check(sm.lib().smh_pool_stats(C.byref(kept), C.byref(live)))
    assert kept.value == 0
    return _used(), live.value


def _exercise(rng, kind):
    if kind == 0:    # banded rows: ring + 16-bit columns
        n = 60_000
        lens = rng.integers(10, 40, n)
        off = np.zeros(n + 1, np.uint32)
        np.cumsum(lens, out=off[1:])
        centers = np.repeat(np.arange(n), lens)
        col = np.clip(centers + rng.integers(-2000, 2000, len(centers)), 0, n - 1).astype(np.uint32)
        val = rng.uniform(-1, 1, len(col)).astype(np.float32)
        n_cols = n
    elif kind == 1:  # stencil: K1s codes, banded ring when the vector family is forced
        g = (120, 110, 12)
        off, col, val = oracle.laplace3d(*g, np.float64)
        n = n_cols = g[0] * g[1] * g[2]
    else:            # random columns: merge, K2c with a small block width
        n, n_cols = 30_000, 50_000
        off, col, val = random_crs(rng, n, n_cols, rng.integers(0, 30, n), np.float32)
    m = sm.SparseMatCRS.from_raw_parts(n, n_cols, off, col, val)
    x = rng.uniform(-1, 1, n_cols).astype(val.dtype)
    m.set_colblock_shift(12)  # at most 39 column blocks for these sizes
    variants = ("auto", "vector", "merge", "stream", "colblock", "colfused", "colsplit", "tiled", "seq")
    for variant in variants:
        m.mvp(x, variant=variant)
    m.set_vector_lanes(4)
    m.mvp(x, variant="vector")
    m.inner_prod(np.ones(n, val.dtype), x)
    m.sort_rows()
    m.mvp(x, variant="auto")
    # every derived form dropped and built again, several times inside one handle's life: new values, a scale, another block width
    s_col, _ = oracle.crs_sort_rows(off, col, val)
    fresh = rng.uniform(-1, 1, len(val)).astype(val.dtype)
    m.update_values(fresh)
    for variant in variants:
        m.mvp(x, variant=variant)
    m.scale(0.5)  # (a power of two: the expected values below are exact)
    for variant in variants:
        m.mvp(x, variant=variant)
    m.set_colblock_shift(13)
    s_val = fresh * val.dtype.type(0.5)
    for variant in variants:
        assert_spmv_close(m.mvp(x, variant=variant), off, s_col, s_val, x, "kind %d, %s after sort / update / scale / shift" % (kind, variant))
    t = sm.SparseMatCRS.from_triplets(rng.integers(0, 500, 5000), rng.integers(0, 400, 5000),
                                      rng.uniform(-1, 1, 5000).astype(np.float32))
    t.sort_rows()
    del m, t


def _with_env(name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def _banded(rng, n, lo, hi):
    """n rows of lo..hi - 1 distinct columns in a band around the diagonal (wrapping): ~(lo + hi) / 2 * n entries"""
    lens = rng.integers(lo, hi, n)
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    k = np.arange(off[-1]) - np.repeat(off[:-1].astype(np.int64), lens)
    col = ((np.repeat(np.arange(n), lens) + 7 * k - 40 + rng.integers(0, 7, len(k))) % n).astype(np.uint32)
    val = rng.uniform(-1, 1, len(col)).astype(np.float32)
    return sm.SparseMatCRS.from_raw_parts(n, int(col.max()) + 1, off, col, val), off, col


def _exercise_matrix_ops(rng):
    # ~320 k entries: the column and value arrays are pooled blocks (1 MiB and more)
    n = 40_000
    a, off, col = _banded(rng, n, 4, 12)
    b, _, _ = _banded(rng, n, 2, 6)
    t = a.transpose()
    assert sm.SparseMatCRS.last_transpose_route() == "bucketed"
    t2 = _with_env("SMH_TRANSPOSE_BUCKETED", "0", a.transpose)
    assert sm.SparseMatCRS.last_transpose_route() == "general"
    p = a.prod(t)
    a.column_info()
    c = a.clone()
    s = a + c
    assert sm.SparseMatCRS.last_add_route() == "same_pattern"
    first = sm.SparseMatCRS.from_raw_parts(n, a.n_cols(), np.arange(n + 1, dtype=np.uint32), col[off[:-1]],
                                           np.ones(n, np.float32))
    c += first
    assert sm.SparseMatCRS.last_add_route() == "structure_unchanged"
    d = a + b
    assert sm.SparseMatCRS.last_add_route() == "short_rows"
    c -= b
    e = _with_env("SMH_ADD_FAST", "0", lambda: a - b)
    assert sm.SparseMatCRS.last_add_route() == "general"
    pick = rng.integers(0, len(col), 100_000)
    rows = np.searchsorted(off, pick, side="right") - 1
    c.apply(rows, col[pick], rng.uniform(-1, 1, len(pick)).astype(np.float32), rng.integers(0, 2, len(pick)))
    assert sm.SparseMatCRS.last_apply_route() == "values_only"
    c.apply(rng.integers(0, n + 100, 100_000), rng.integers(0, n, 100_000), rng.uniform(-1, 1, 100_000).astype(np.float32))
    assert sm.SparseMatCRS.last_apply_route() == "general"
    _with_env("SMH_APPLY_FAST", "0", lambda: d.apply(rows, col[pick], np.ones(len(pick), np.float32)))
    assert sm.SparseMatCRS.last_apply_route() == "general"
    a.get_many(rng.integers(0, n, 300_000), rng.integers(0, n, 300_000))
    i = sm.SparseMatCRS.eye(300_000)
    r = sm.SparseMatCRS.from_triplets(rng.integers(0, 20_000, 300_000), rng.integers(0, 20_000, 300_000),
                                      rng.uniform(-1, 1, 300_000).astype(np.float32), into_crs=True)
    del a, b, t, t2, p, c, s, first, d, e, i, r


PAR_GRID = 84   # 592 704 rows in two blocks: a block's full-length vectors AND its per-block arrays (r, Ap: ~296 k entries) are
PAR_ITERS = 5   # pooled blocks (1 MiB and more) in f32 already, so the exact comparison of live bytes sees them
_stencils = {}


def _stencil(dtype):
    if dtype not in _stencils:
        _stencils[dtype] = oracle.laplace3d(PAR_GRID, PAR_GRID, PAR_GRID, dtype)
    return _stencils[dtype]


def _exercise_par(rng, dtype):
    """Two blocks on one device, cut by rows, by entries, and adopted from existing blocks; the host-vector product, the
    device-resident one with both exchanges (overlap and issuing threads on and off), user vectors, both solvers.  Returns
    what the oracle is asked about after the last round."""
    off, col, val = _stencil(dtype)
    n = PAR_GRID ** 3
    x = rng.uniform(-1, 1, n).astype(dtype)
    b = rng.uniform(-1, 1, n).astype(dtype)
    by_rows = sm.SparseMatParLocal.with_sub_matrices(2, n, n, off, col, val, device_ids=[0, 0])
    by_nnz = sm.SparseMatParLocal.with_sub_matrices(2, n, n, off, col, val, device_ids=[0, 0], split="nnz")
    cut = by_nnz.split()
    blocks = []
    for k in range(2):
        o = off[cut[k]:cut[k + 1] + 1].astype(np.int64)
        blocks.append(sm.SparseMatCRS.from_raw_parts(cut[k + 1] - cut[k], n, (o - o[0]).astype(np.uint32), col[o[0]:o[-1]], val[o[0]:o[-1]]))
    adopted = sm.SparseMatParLocal.adopt(blocks, n, split_rows=cut)
    out = {"x": x, "b": b, "mvp": by_rows.mvp(x, variant="stream"), "mvp_dev": []}
    xv, yv = by_nnz.vec(host=x), by_nnz.vec()
    for exchange in ("allgather", "window"):
        for overlap in (True, False):
            for threads in (1, 0):
                by_nnz.set_overlap(overlap)
                by_nnz.set_threads(threads)
                by_nnz.mvp_dev(xv, yv, variant="stream", exchange=exchange)
                out["mvp_dev"].append(yv.download())
    xv.close()
    yv.close()
    out["cg"] = np.zeros(n, dtype)
    by_rows.cg_solve(b, out["cg"], tol=0.0, iter_max=PAR_ITERS)
    bv, sv = adopted.vec(host=b), adopted.vec()
    adopted.cg_solve_vec(bv, sv, tol=0.0, iter_max=PAR_ITERS, check_every=2)
    out["cg_vec"] = sv.download()
    bv.close()
    sv.close()
    for m in (by_rows, by_nnz, adopted):
        m.close()
    del blocks
    return out


def _exercise_solvers(rng, dtype, out):
    """The single-matrix solvers on the same stencil and right-hand side (every vector of theirs is a pooled block): replayed
    batches, plain launches, a solve that fails after its workspaces exist, calls that fail before anything is allocated."""
    off, col, val = _stencil(dtype)
    n = PAR_GRID ** 3
    b = out["b"]
    a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    cg = sm.ConjugateGradient(0.0, PAR_ITERS)  # 4 bodies per poll: two replayed batches
    out["cg_single"] = cg.solve(a, b, np.zeros(n, dtype))
    assert cg.iterations == PAR_ITERS
    bv, xv = sm.DenseVec.from_vec(b), sm.DenseVec.zeros(n, dtype)
    cg = sm.ConjugateGradient(0.0, PAR_ITERS, check_every=7)  # more bodies per poll than there are: plain launches
    cg.solve(a, bv, xv)
    assert cg.iterations == PAR_ITERS
    out["cg_single_vec"] = xv.to_numpy()
    pcg = sm.JacobiConjugateGradient(0.0, 9)  # a replayed batch of 8 and one more
    pcg.solve(a, b, np.zeros(n, dtype))
    assert pcg.iterations == 9
    # a zero on the diagonal: found when the vectors, the scalar blocks and the stream of the solve exist
    nd = 300_000
    row = int(rng.integers(0, nd))
    dval = np.ones(nd, np.float32)
    dval[row] = 0
    d = sm.SparseMatCRS.from_raw_parts(nd, nd, np.arange(nd + 1, dtype=np.uint32), np.arange(nd, dtype=np.uint32), dval)
    with pytest.raises(sm.SparseMatPanic) as e:
        sm.JacobiConjugateGradient().solve(d, np.ones(nd, np.float32), np.zeros(nd, np.float32))
    assert str(e.value) == "Jacobi preconditioner: zero or absent diagonal entry in row %d" % row
    for solver in (sm.ConjugateGradient(), sm.JacobiConjugateGradient()):
        with pytest.raises(sm.SparseMatPanic) as e:   # linearsolver.rs:33-36
            solver.solve(a, b[:-1], np.zeros(n, dtype))
        assert e.value.status == _lib.SMH_ERR_DIM_MISMATCH and "Matrix and vector size mismatch" in str(e.value)
    del e, a, d, bv, xv


def _check_par(dtype, out):
    """The last round's products and iterates against the oracle: the round did what it says."""
    off, col, val = _stencil(dtype)
    n = PAR_GRID ** 3
    assert_spmv_close(out["mvp"], off, col, val, out["x"], "partitioned mvp, %s" % np.dtype(dtype).name)
    assert_spmv_close(out["mvp_dev"][0], off, col, val, out["x"], "partitioned mvp_dev, %s" % np.dtype(dtype).name)
    for y in out["mvp_dev"][1:]:  # (tests/test_par_overlap_gpu.py: the exchange, the overlap and the threads do not touch a bit)
        assert y.tobytes() == out["mvp_dev"][0].tobytes()
    # PAR_ITERS iterations from x = 0 on both sides.  The two differ in the order of their sums only: the oracle's dot products
    # are serial, the device's are trees over blocks.  A sum of n terms carries a relative rounding error of about sqrt(n) eps
    # (the errors of its additions accumulate as a random walk); each iteration feeds two such sums (p.Ap, r.r) into alpha and
    # beta, and x inherits their errors linearly.  A factor 8 on top for the products' and the vector updates' own rounding.
    want, iters, _ = oracle.cg(n, n, off, col, val, out["b"], np.zeros(n, dtype), tol=0.0, iter_max=PAR_ITERS)
    assert iters == PAR_ITERS
    bound = 8 * PAR_ITERS * 2 * np.sqrt(n) * np.finfo(dtype).eps * np.abs(want).max()
    for name in ("cg", "cg_vec", "cg_single", "cg_single_vec"):  # (partitioned; one matrix: the same recurrence, the same bound)
        err = np.abs(out[name].astype(np.float64) - want.astype(np.float64)).max()
        print("%s, %s: max |x - x_oracle| = %.3e (bound %.3e)" % (name, np.dtype(dtype).name, err, bound))
        assert err <= bound, (name, err, bound)


def _round(rng):
    for kind in range(3):
        _exercise(rng, kind)
    _exercise_matrix_ops(rng)
    last = {}
    for dtype in (np.float32, np.float64):
        last[dtype] = _exercise_par(rng, dtype)
        _exercise_solvers(rng, dtype, last[dtype])
    return last


def test_no_device_memory_is_left_behind(gpu):
    rng = np.random.default_rng(0)
    _round(rng)  # first round: one-time allocations (code objects, rocPRIM state, thread-local scratch)
    gc.collect()
    # the library keeps the device memory it frees (csrc/pool.hip): what it KEEPS depends on what ran before in this process, so both
    # readings are taken with the pool returned to the runtime, and the bytes the library has handed out are compared exactly
    before, live_before = _used_without_the_pool()
    for rep in range(8):
        last = _round(rng)
    gc.collect()
    after, live_after = _used_without_the_pool()
    assert live_after == live_before, "the library still holds %d bytes more than before" % (live_after - live_before)
    assert after - before < 8 << 20, "device memory in use grew by %.1f MiB over 8 create/use/destroy rounds" % ((after - before) / 2 ** 20)
    for dtype, out in last.items():
        _check_par(dtype, out)
