"""tests/cg_model.py pinned without a GPU: in "sequential" mode its two recurrences are the oracle's (orc_cg_*,
orc_pcg_jacobi_*: the project's restatement of the reference) bit for bit, and its "device" trees sum what they are given
(a slip in a tree -- a lane dropped, an element counted twice -- shows against an exact sum)."""
import math

import numpy as np
import pytest

import cg_model
import oracle

DTYPES = [np.float32, np.float64]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    """bit equality, any NaN equal to any NaN (its sign and payload are the host's business)"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def system(name, dtype):
    if name == "laplace":
        off, col, val = oracle.laplace3d(7, 11, 13, dtype)
    elif name == "scaled":
        off, col, val = cg_model.tridiag(259, dtype, seed=4, spread=2.0)
    else:
        off, col, val = cg_model.tridiag(int(name), dtype, seed=3)
    n = len(off) - 1
    rng = np.random.default_rng(n + 7)
    b = rng.uniform(-1, 1, n).astype(dtype)
    x_rand = rng.uniform(-1, 1, n).astype(dtype)
    return n, off, col, val, b, x_rand


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["0", "1", "2", "5", "257", "laplace", "scaled"])
@pytest.mark.parametrize("x0_kind", ["zero", "random"])
@pytest.mark.parametrize("solver", ["cg", "pcg"])
def test_sequential_model_is_the_oracle(solver, x0_kind, name, dtype):
    n, off, col, val, b, x_rand = system(name, dtype)
    x0 = np.zeros(n, dtype) if x0_kind == "zero" else x_rand
    model = cg_model.cg if solver == "cg" else cg_model.pcg
    orc = oracle.cg if solver == "cg" else oracle.pcg_jacobi
    # tol = 0: iter_max bodies; then a tol that only the smallest of the first eight residual norms passes: the loop has
    # to leave in that body (mid-way unless the norms only grow), with that body's x
    full = model(off, col, val, b, x0, 0.0, 9, mode="sequential")
    norms = [math.sqrt(float(v)) for v in full.rr_list]
    tols = [0.0]
    if n > 5:
        order = np.argsort(norms[:8])
        k = int(order[0])
        assert norms[k] < norms[order[1]]
        tols.append(0.5 * (norms[k] + norms[order[1]]))
    for tol in tols:
        for iter_max in (0, 1, 9):
            got = model(off, col, val, b, x0, tol, iter_max, mode="sequential")
            o_x, o_iters, o_rr = orc(n, n, off, col, val, b, x0, tol=tol, iter_max=iter_max)
            assert got.iterations == o_iters, (tol, iter_max)
            assert same(got.x, o_x), (tol, iter_max)
            assert same(np.float64(got.r_norm_squared), np.float64(o_rr)), (tol, iter_max)
    if n > 5:
        stopped = model(off, col, val, b, x0, tols[1], 9, mode="sequential")
        assert stopped.iterations == k + 1 < 9


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("solver", ["cg", "pcg"])
def test_breakdown_and_empty_system_like_the_oracle(solver, dtype):
    """b = 0: alpha = 0 / 0, x fills with NaN, iter_max bodies (no breakdown guard, linearsolver.rs:45); n = 0: one body."""
    model = cg_model.cg if solver == "cg" else cg_model.pcg
    orc = oracle.cg if solver == "cg" else oracle.pcg_jacobi
    for mode in ("sequential", "device"):
        off, col, val = cg_model.tridiag(37, dtype, seed=1)
        z = np.zeros(37, dtype)
        got = model(off, col, val, z, z, 1e-6, 5, mode=mode)
        o_x, o_iters, o_rr = orc(37, 37, off, col, val, z, z, tol=1e-6, iter_max=5)
        assert got.iterations == o_iters == 5 and np.isnan(o_rr) and np.isnan(got.r_norm_squared)
        assert np.array_equal(np.isnan(got.x), np.isnan(o_x)) and np.isnan(o_x).all()
        off, col, val = cg_model.tridiag(0, dtype)
        e = np.zeros(0, dtype)
        got = model(off, col, val, e, e, 1e-6, 5, mode=mode)
        _, o_iters, o_rr = orc(0, 0, off, col, val, e, e, tol=1e-6, iter_max=5)
        assert (got.iterations, got.r_norm_squared) == (o_iters, o_rr) == (1, 0.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 3, 5, 255, 257, 2049, 2051, 131_072 + 259, 300_003])
def test_device_trees_sum_their_terms(n, dtype):
    """Every tree of the "device" mode against math.fsum of the same (already rounded) terms, within
    (chain length + tree depth) * eps * sum|t_i| (each addition a term passes through costs at most one relative eps/2;
    tree_depth counts them along the longest path)."""
    rng = np.random.default_rng(n)
    x, y = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
    terms = x * y
    exact = math.fsum(terms.astype(np.float64).tolist())
    scale = math.fsum(np.abs(terms).astype(np.float64).tolist())
    eps = float(np.finfo(dtype).eps)
    V = cg_model.vec_len(dtype)
    for grid, v, first in ((cg_model.reduce_blocks(n), V, False), (cg_model.cg_update_grid(n), V, False),
                           (cg_model.cg_update_grid(n), 1, False), (cg_model.pcg_grid(n), V, True)):
        got = cg_model.device_sum(terms, grid, v, from_first=first)
        assert got.dtype == np.dtype(dtype)
        assert abs(float(got) - exact) <= cg_model.tree_depth(n, grid, v) * eps * scale, (grid, v, first)
    # a term of its own magnitude cannot be lost: one huge element in the tail / the last lane / the last workgroup
    for pos in (n - 1, n // 2, 0):
        t = np.zeros(n, dtype)
        t[pos] = 3.0
        for grid, v, first in ((cg_model.reduce_blocks(n), V, False), (cg_model.cg_update_grid(n), 1, False),
                               (cg_model.pcg_grid(n), V, True)):
            assert cg_model.device_sum(t, grid, v, from_first=first) == 3.0, (pos, grid, v)
    # the Reducer's modes agree to rounding, and "wide" is the correctly rounded sum
    dots = {m: float(cg_model.Reducer(m).dot(x, y, "dot")) for m in ("sequential", "device", "wide")}
    wide_exact = math.fsum((x.astype(np.float64) * y.astype(np.float64)).tolist()) if dtype == np.float32 else None
    if wide_exact is not None:
        assert dots["wide"] == float(np.float32(wide_exact))
    for m in ("sequential", "device"):
        assert abs(dots[m] - dots["wide"]) <= (n + 2) * eps * scale


def test_diagonal_takes_the_first_match_in_storage_order():
    off = np.array([0, 3, 5, 6], np.uint32)
    col = np.array([2, 0, 0, 1, 1, 0], np.uint32)   # row 0: (2, 0, 0) -> first 0; row 1: (1, 1) -> first; row 2: no diagonal
    val = np.array([9.0, 4.0, 5.0, 6.0, 7.0, 8.0])
    assert cg_model.diagonal(off, col, val).tolist() == [4.0, 6.0, 0.0]


class CountedProduct:
    """oracle.spmv as a ``product`` callable that counts its calls; bump = (c, k): in the c-th call the element of k-th largest
    magnitude moves by one ulp."""

    def __init__(self, off, col, val, bump=(None, 0)):
        self.parts, self.bump, self.calls = (off, col, val), bump, 0

    def __call__(self, v):
        y = oracle.spmv(*self.parts, v)
        if self.calls == self.bump[0]:
            j = int(np.argsort(-np.abs(y), kind="stable")[self.bump[1]])
            y[j] = np.nextafter(y[j], y.dtype.type(np.inf))
        self.calls += 1
        return y


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mode", ["sequential", "device", "wide"])
@pytest.mark.parametrize("solver", ["cg", "pcg"])
def test_product_callable_is_what_the_model_consumes(solver, mode, dtype):
    """product = the oracle's own product: the default's bytes (x, every r.r, the body count), 1 + bodies calls (the initial
    residual's and one per entered body; fewer bodies after a stop on tol).  One ulp on one element of ANY single call --
    the initial residual's included -- changes the result (x, r, p or an r.r: one ulp on one element seldom moves a dot of a
    thousand terms, so the last call's shows in r and p alone): no product is taken from anywhere else.  (It can also round
    away in Ap * alpha, so for each call the elements are tried in order of magnitude, at most eight of them, until one
    shows.)  The fused p.Ap reads the callable's Ap too."""
    n, off, col, val, b, x0 = system("laplace", dtype)
    model = cg_model.cg if solver == "cg" else cg_model.pcg
    bodies = 5
    for fused in ((False, True) if mode == "device" else (False,)):
        for tol in (0.0, None):
            want = model(off, col, val, b, x0, 0.0, bodies, mode=mode, fused=fused)
            if tol is None:  # a stop on tol in body 3
                tol = 0.5 * (math.sqrt(float(want.rr_list[2])) + min(math.sqrt(float(v)) for v in want.rr_list[:2]))
                want = model(off, col, val, b, x0, tol, bodies, mode=mode, fused=fused)
                assert want.iterations == 3
            counted = CountedProduct(off, col, val)
            got = model(off, col, val, b, x0, tol, bodies, mode=mode, fused=fused, product=counted)
            assert counted.calls == 1 + want.iterations
            assert got.iterations == want.iterations and same(got.x, want.x) and same(got.rr, want.rr)
            assert same(np.array(got.rr_list), np.array(want.rr_list)) and same(got.r, want.r) and same(got.p, want.p)
        plain = model(off, col, val, b, x0, 0.0, bodies, mode=mode, fused=fused)
        for call in range(1 + bodies):
            for k in range(8):
                bumped = model(off, col, val, b, x0, 0.0, bodies, mode=mode, fused=fused, product=CountedProduct(off, col, val, bump=(call, k)))
                if not all(same(u, v) for u, v in ((bumped.x, plain.x), (bumped.r, plain.r), (bumped.p, plain.p),
                                                   (np.array(bumped.rr_list), np.array(plain.rr_list)))):
                    break
            else:
                raise AssertionError("call %d of the product is not consumed (fused %s)" % (call, fused))
