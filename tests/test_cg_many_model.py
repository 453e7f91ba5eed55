"""tests/cg_many_model.py pinned without a GPU: in "sequential" mode every column of the k-column recurrence is the oracle's CG
(the project's restatement of the reference's ConjugateGradient::solve) bit for bit -- x, the iteration count, r.r --; "device"
mode does not let the set of columns, or their order, reach a column; the binding declares the new entry points."""
import json
import math
import os

import numpy as np
import pytest

import cg_many_model
import cg_model
import oracle
from sparsemat_amd import _lib

DTYPES = [np.float32, np.float64]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    """bit equality, any NaN equal to any NaN"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def system(name, dtype, k=4):
    if name == "laplace":
        off, col, val = oracle.laplace3d(5, 7, 3, dtype)
    else:
        off, col, val = cg_model.tridiag(int(name), dtype, seed=3)
    n = len(off) - 1
    rng = np.random.default_rng(n + 11)
    B = rng.uniform(-1, 1, (k, n)).astype(dtype) * (10.0 ** -np.arange(k))[:, None].astype(dtype)
    X0 = rng.uniform(-1, 1, (k, n)).astype(dtype)
    return n, off, col, val, B, X0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["0", "1", "2", "5", "257", "laplace"])
@pytest.mark.parametrize("x0_kind", ["zero", "random"])
def test_sequential_columns_are_the_oracle(x0_kind, name, dtype):
    n, off, col, val, B, X0 = system(name, dtype)
    if x0_kind == "zero":
        X0 = np.zeros_like(X0)
    for tol, iter_max in ((0.0, 0), (0.0, 1), (0.0, 7), (1e-3, 30)):
        got = cg_many_model.cg_many(off, col, val, B, X0, tol, iter_max, mode="sequential")
        assert got.x.shape == B.shape and got.iterations.shape == (4,) and got.r_norm_squared.dtype == np.float64
        for c in range(4):
            o_x, o_iters, o_rr = oracle.cg(n, n, off, col, val, B[c], X0[c], tol=tol, iter_max=iter_max)
            assert got.iterations[c] == o_iters, (tol, iter_max, c)
            assert same(got.x[c], o_x), (tol, iter_max, c)
            assert same(np.float64(got.r_norm_squared[c]), np.float64(o_rr)), (tol, iter_max, c)
    if n > 5 and x0_kind == "zero":  # the scaled right-hand sides really stop in different bodies
        assert len(set(cg_many_model.cg_many(off, col, val, B, X0, 1e-3, 30, mode="sequential").iterations.tolist())) >= 2


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_sequential_known_answer_of_the_reference(dtype):
    """check_cg (src/lib.rs:36-52) as one column among others: floor(x0 * 1e4) / 1e4 == 0.0909 in f64, and the oracle's bits."""
    case = [c for c in json.load(open(GOLDEN))["cases"] if c["name"] == "check_cg"][0]
    crs = case["crs"]
    off, col = np.array(crs["offset_rows"], np.uint32), np.array(crs["columns"], np.uint32)
    val = np.array([int(b, 16) for b in crs["values_bits"]], np.uint64).view(np.float64).astype(dtype)
    b = np.array([float(s) for s in case["b"]], dtype)
    x0 = np.array([float(s) for s in case["x0"]], dtype)
    tol = case["cg"]["tol"] if dtype == np.float64 else 1e-6
    B, X0 = np.stack([b[::-1], b, 3 * b]), np.stack([x0, x0, np.zeros(2, dtype)])
    got = cg_many_model.cg_many(off, col, val, B, X0, tol, case["cg"]["iter_max"], mode="sequential")
    for c in range(3):
        o_x, o_iters, o_rr = oracle.cg(2, 2, off, col, val, B[c], X0[c], tol=tol, iter_max=case["cg"]["iter_max"])
        assert got.iterations[c] == o_iters and same(got.x[c], o_x) and same(np.float64(got.r_norm_squared[c]), np.float64(o_rr))
    if dtype == np.float64:
        for i, lit in case["expect_floor_1e4"]:
            assert np.floor(got.x[1][i] * 1e4) / 1e4 == float(lit)
        assert got.iterations[1] == 2 and math.sqrt(got.r_norm_squared[1]) < 1e-12


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [5, 257, 2051])
def test_device_mode_is_invariant_under_the_set_of_columns(n, dtype):
    off, col, val = cg_model.tridiag(n, dtype, seed=5)
    rng = np.random.default_rng(n)
    B = rng.uniform(-1, 1, (5, n)).astype(dtype)
    B[2] = 0   # a NaN recurrence among them
    X0 = rng.uniform(-1, 1, (5, n)).astype(dtype)
    X0[2] = 0
    full =cg_many_model.cg_many(off, col, val, B, X0, 1e-4, 6)
    for pick in ([0], [4, 3, 2, 1, 0], [1, 3], [3, 3, 0, 2], [0, 1, 2, 3, 4, 0, 1]):   # removed, permuted, repeated, added
        got = cg_many_model.cg_many(off, col, val, B[pick], X0[pick], 1e-4, 6)
        for j, c in enumerate(pick):
            assert same(got.x[j], full.x[c]) and got.iterations[j] == full.iterations[c]
            assert same(got.r_norm_squared[j], full.r_norm_squared[c])
    assert full.iterations[2] == 6 and np.isnan(full.x[2]).all() and not np.isnan(np.delete(full.x, 2, 0)).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_column_sum_is_the_documented_tree(dtype):
    """column_sum against the tree written out by hand for a size with two workgroups and a ragged last stride, and against an
    exact sum within the tree's error bound."""
    n = 2 * 2048 + 77
    G = cg_model.cg_update_grid(n)
    assert G == 3
    rng = np.random.default_rng(9)
    t = rng.uniform(-1, 1, n).astype(dtype)
    T = np.dtype(dtype).type
    acc = np.zeros(G * 256, dtype)
    for i in range(n):   # thread g takes rows g, g + 256 G, ...
        acc[i % (G * 256)] = acc[i % (G * 256)] + t[i]

    def wg(v):   # 256 values -> the workgroup sum
        waves = []
        for w in range(4):
            lane = v[64 * w:64 * w + 64].copy()
            o = 32
            while o:
                lane[:o] = lane[:o] + lane[o:2 * o]
                o //= 2
            waves.append(lane[0])
        r = T(0)
        for s in waves:
            r = r + s
        return r

    partials = np.array([wg(acc[256 * w:256 * w + 256]) for w in range(G)], dtype)
    fold = np.zeros(256, dtype)
    fold[:G] = partials
    want = wg(fold)
    got = cg_many_model.column_sum(t)
    assert same(got, want)
    exact = math.fsum(t.astype(np.float64).tolist())
    assert abs(float(got) - exact) <= cg_model.tree_depth(n, G, 1) * np.finfo(dtype).eps * np.abs(t).sum()
    assert same(cg_many_model.column_sum(t, "sequential"), cg_model.sequential_sum(t))
    assert same(cg_many_model.column_sum(np.zeros(0, dtype)), T(0))


def test_binding_declares_the_new_entry_points():
    want = {
        "smh_mvec_copy": 2, "smh_mvec_add": 2, "smh_mvec_sub": 2, "smh_mvec_scale": 2, "smh_mvec_dot": 3, "smh_mvec_norm_squared": 2,
        "smh_cg_solve_many": 8, "smh_cg_solve_many_host": 9,
    }
    for name, n_args in want.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sparsemat_hip.h")).read()
    for name in want:
        assert name + "(" in header, name
