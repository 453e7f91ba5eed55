"""GPU parity of the DenseVec kernels (K3/K4) and the device-resident CG (K5) against the oracle."""
import json
import os

import numpy as np
import pytest

import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [0, 1, 3, 64, 1023, 4096 + 5, 300_001])
def test_elementwise_bit_exact(gpu, dtype, n):
    """densevec.rs:51-73 and the composite updates of linearsolver.rs:47,58-59: one rounding per
    multiply and per add -> bit-identical to the oracle."""
    rng = np.random.default_rng(n + 1)
    a, b = rng.uniform(-2, 2, n).astype(dtype), rng.uniform(-2, 2, n).astype(dtype)
    s = dtype(0.7310585786300049)
    bits = np.uint32 if dtype == np.float32 else np.uint64

    def same(got, want):
        assert np.array_equal(got.view(bits), want.view(bits))

    x, y = sm.DenseVec.from_vec(a), sm.DenseVec.from_vec(b)
    assert x.dim() == n
    x.add(y); same(x.to_numpy(), oracle.vec_add(a, b))
    x = sm.DenseVec.from_vec(a); x.sub(y); same(x.to_numpy(), oracle.vec_sub(a, b))
    x = sm.DenseVec.from_vec(a); x.scale(s); same(x.to_numpy(), oracle.vec_scale(a, s))
    x = sm.DenseVec.from_vec(a); x.axpy(s, y); same(x.to_numpy(), oracle.vec_axpy(a, s, b))
    x = sm.DenseVec.from_vec(a); x.xpby(s, y); same(x.to_numpy(), oracle.vec_xpby(a, s, b))
    # operator sugar (densevec.rs:76-130) leaves the operands untouched
    x = sm.DenseVec.from_vec(a)
    same((x + y).to_numpy(), oracle.vec_add(a, b))
    same((x - y).to_numpy(), oracle.vec_sub(a, b))
    same((x * s).to_numpy(), oracle.vec_scale(a, s))
    same(x.to_numpy(), a)


def test_elementwise_shorter_rhs_and_mismatch(gpu):
    """zip truncation and the "Dimension mismatch" panic (densevec.rs:52-54)."""
    a, b = np.arange(10, dtype=np.float32), np.ones(4, dtype=np.float32)
    x, y = sm.DenseVec.from_vec(a), sm.DenseVec.from_vec(b)
    x.add(y)
    assert np.array_equal(x.to_numpy(), oracle.vec_add(a, b))
    with pytest.raises(sm.SparseMatPanic) as e:
        y.add(x)
    assert e.value.status == _lib.SMH_ERR_DIM_MISMATCH and "Dimension mismatch" in str(e.value)
    with pytest.raises(oracle.OraclePanic):
        oracle.vec_add(b, a)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [0, 1, 5, 255, 256, 257, 70_001, 3_000_017])
def test_reductions(gpu, dtype, n):
    """vector.rs:50-63.  The reference folds left to right in T; the device uses a fixed tree in T.
    Both are within n*eps*sum|x_i y_i| of the exact value; the tree is bitwise reproducible."""
    rng = np.random.default_rng(n + 17)
    a, b = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
    x, y = sm.DenseVec.from_vec(a), sm.DenseVec.from_vec(b)
    eps = np.finfo(dtype).eps
    exact = float(np.dot(a.astype(np.float64), b.astype(np.float64)))
    scale = float(np.dot(np.abs(a).astype(np.float64), np.abs(b).astype(np.float64)))
    d = x.inner_prod(y)
    assert isinstance(d, dtype)
    assert abs(float(d) - exact) <= (np.log2(max(n, 2)) + 8) * eps * scale + 1e-300
    ref = oracle.dot(a, b)
    assert abs(float(d) - float(ref)) <= 2 * max(n, 1) * eps * scale + 1e-300
    assert x.inner_prod(y) == d and (x * y) == d  # reproducible; `v * w` sugar (densevec.rs:133-140)
    nn = x.norm_squared()
    assert abs(float(nn) - float(oracle.norm_squared(a))) <= 2 * max(n, 1) * eps * float(np.dot(a.astype(np.float64), a.astype(np.float64))) + 1e-300
    assert x.norm() == np.sqrt(float(nn))


def test_cg_reference_known_answer(gpu):
    """check_cg (src/lib.rs:36-52): 2x2 f64, default CG -> floor(x0*1e4)/1e4 == 0.0909."""
    with open(GOLDEN) as f:
        case = [c for c in json.load(f)["cases"] if c["name"] == "check_cg"][0]
    crs = case["crs"]
    val = np.array(crs["values"], dtype=np.float64)
    m = sm.SparseMatCRS.from_raw_parts(crs["n_rows"], crs["n_cols"], crs["offset_rows"], crs["columns"], val)
    b = np.array([float(s) for s in case["b"]])
    for variant in ("seq", "vector", "merge", "auto"):
        x = np.array([float(s) for s in case["x0"]])
        cg = sm.ConjugateGradient.default()
        cg.variant = variant
        cg.solve(m, b, x)
        assert np.floor(x[0] * 1e4) / 1e4 == float(case["expect_floor_1e4"][0][1])
        x_ref, it_ref, _ = oracle.cg(2, 2, crs["offset_rows"], crs["columns"], val, b, [2.0, 1.0])
        assert cg.iterations == it_ref == 2
        np.testing.assert_allclose(x, x_ref, rtol=1e-14)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-9), (np.float32, 1e-3)], ids=["f64", "f32"])
def test_cg_laplace3d_matches_oracle(gpu, dtype, tol):
    """SPD 7-point Laplacian, b = A.1, x0 = 0, reference stop rule (linearsolver.rs:52)."""
    nx = ny = nz = 12
    n = nx * ny * nz
    off, col, val = oracle.laplace3d(nx, ny, nz, dtype)
    b = oracle.spmv(off, col, val, np.ones(n, dtype))
    x_ref, it_ref, rr_ref = oracle.cg(n, n, off, col, val, b, np.zeros(n, dtype), tol=tol, iter_max=500)
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    for variant in ("seq", "auto", "merge", "vector", "tiled", "colblock"):
        for check_every in (1, 7):
            x = np.zeros(n, dtype)
            xd, bd = sm.DenseVec.from_vec(x), sm.DenseVec.from_vec(b)
            cg = sm.ConjugateGradient(tol, 500, variant=variant, check_every=check_every)
            cg.solve(m, bd, xd)
            # measured (tools/dev/cg_probe.py, r02): every kernel family stops in the oracle's iteration, |x - x_ref| <= 0.03 tol
            assert abs(cg.iterations - it_ref) <= 1, (variant, cg.iterations, it_ref)
            assert np.sqrt(cg.r_norm_squared) < tol
            np.testing.assert_allclose(xd.to_numpy(), x_ref, rtol=0, atol=10 * tol)
            np.testing.assert_allclose(xd.to_numpy(), np.ones(n), rtol=0, atol=10 * tol)


def test_cg_64_cubed_f64_convergence_parity(gpu):
    """the 64^3 f64 convergence-parity case with the reference stop rule (sqrt(r.r) < tol, absolute,
    tested before the beta update): same iteration count as the oracle (+-1: the reductions are regrouped; measured 195
    on both sides) and the same solution (measured |x - x_ref| < 0.01 tol), for the bit-exact SpMV kernel and for AUTO;
    b = A.1, x0 = 0."""
    g, dtype, tol = 64, np.float64, 1e-9
    n = g ** 3
    off, col, val = oracle.laplace3d(g, g, g, dtype)
    b = oracle.spmv(off, col, val, np.ones(n, dtype))
    x_ref, it_ref, rr_ref = oracle.cg(n, n, off, col, val, b, np.zeros(n, dtype), tol=tol, iter_max=2000)
    assert 50 < it_ref < 2000 and np.sqrt(rr_ref) < tol
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    for variant in ("stream", "auto"):
        xd, bd = sm.DenseVec.from_vec(np.zeros(n, dtype)), sm.DenseVec.from_vec(b)
        cg = sm.ConjugateGradient(tol, 2000, variant=variant)
        cg.solve(m, bd, xd)
        assert abs(cg.iterations - it_ref) <= 1, (variant, cg.iterations, it_ref)
        assert np.sqrt(cg.r_norm_squared) < tol
        np.testing.assert_allclose(xd.to_numpy(), x_ref, rtol=0, atol=10 * tol)
        np.testing.assert_allclose(xd.to_numpy(), np.ones(n), rtol=0, atol=10 * tol)


def test_cg_iter_max_and_exact_iteration_semantics(gpu):
    """iter_max bodies are entered at most; with SEQ SpMV and equal scalars the first iteration is
    bit-identical to the oracle's (element-wise updates round like the reference)."""
    n = 10 * 10 * 10
    off, col, val = oracle.laplace3d(10, 10, 10, np.float64)
    rng = np.random.default_rng(5)
    b = rng.uniform(-1, 1, n)
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    for iters in (0, 1, 3):
        x = np.zeros(n)
        cg = sm.ConjugateGradient(1e-30, iters, variant="seq", check_every=5)
        cg.solve(m, b, x)
        x_ref, it_ref, rr_ref = oracle.cg(n, n, off, col, val, b, np.zeros(n), tol=1e-30, iter_max=iters)
        assert cg.iterations == it_ref == iters
        np.testing.assert_allclose(x, x_ref, rtol=1e-12, atol=1e-14)
        if iters:
            assert abs(cg.r_norm_squared - rr_ref) <= 1e-10 * rr_ref


def test_cg_panics_of_the_reference(gpu):
    f = np.float64
    m = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 2], np.array([1, 2], f))
    with pytest.raises(sm.SparseMatPanic) as e:
        sm.ConjugateGradient().solve(m, np.ones(2), np.zeros(2))
    assert e.value.status == _lib.SMH_ERR_NOT_SQUARE and str(e.value) == "Matrix is not symmetric"
    m = sm.SparseMatCRS.from_raw_parts(2, 2, [0, 1, 2], [0, 1], np.array([1, 2], f))
    with pytest.raises(sm.SparseMatPanic) as e:
        sm.ConjugateGradient().solve(m, np.ones(3), np.zeros(2))
    assert e.value.status == _lib.SMH_ERR_DIM_MISMATCH and str(e.value) == "Matrix and vector size mismatch"
    with pytest.raises(oracle.OraclePanic):
        oracle.cg(2, 2, [0, 1, 2], [0, 1], np.array([1, 2], f), np.ones(3), np.zeros(2))


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-9), (np.float32, 1e-3)], ids=["f64", "f32"])
def test_par_cg_single_rank_matches_oracle(gpu, dtype, tol):
    """ParConjugateGradient (the row-partitioned recurrence, device scalars, smh_blas_*_dev kernels) with one
    block: same iterates as the oracle up to the reduction order."""
    import torch
    from par_reference import HipBlock, ParConjugateGradient, SparseMatPar
    nx = ny = nz = 12
    n = nx * ny * nz
    off, col, val = oracle.laplace3d(nx, ny, nz, dtype)
    b = oracle.spmv(off, col, val, np.ones(n, dtype))
    x_ref, it_ref, _ = oracle.cg(n, n, off, col, val, b, np.zeros(n, dtype), tol=tol, iter_max=500)
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    par = SparseMatPar(1, n, n, 0, HipBlock(m))
    bt = torch.from_numpy(b).cuda()
    xt = torch.zeros(n, dtype=bt.dtype, device="cuda")
    cg = ParConjugateGradient(tol, 500)
    cg.solve(par, bt, xt)
    torch.cuda.synchronize()
    assert abs(cg.iterations - it_ref) <= 2 and np.sqrt(cg.r_norm_squared) < tol
    np.testing.assert_allclose(xt.cpu().numpy(), x_ref, rtol=0, atol=50 * tol)
    # first iteration is bit-identical to the oracle's when the SpMV is a bit-exact kernel (AUTO = K1s here)
    xt1 = torch.zeros(n, dtype=bt.dtype, device="cuda")
    ParConjugateGradient(0.0, 1).solve(par, bt, xt1)
    x1, _, _ = oracle.cg(n, n, off, col, val, b, np.zeros(n, dtype), tol=0.0, iter_max=1)
    np.testing.assert_allclose(xt1.cpu().numpy(), x1, rtol=1e-6 if dtype == np.float32 else 1e-14)
    with pytest.raises(sm.SparseMatPanic):
        cg.solve(par, bt[:-1], xt)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", ["laplace", "rect_ragged", "powerlaw"])
def test_matrix_inner_prod(gpu, dtype, shape):
    """SparseMatrix::inner_prod (sparsematrix.rs:161-171) = lhs^T A rhs: within eps * n-ish of the oracle's
    sequential sum, relative to sum |lhs_i a_ij rhs_j| (a reduction: tolerance-level, like dot)."""
    rng = np.random.default_rng({"laplace": 1, "rect_ragged": 2, "powerlaw": 3}[shape])
    if shape == "laplace":
        off, col, val = oracle.laplace3d(23, 17, 9, dtype)
        n_rows = n_cols = 23 * 17 * 9
    elif shape == "rect_ragged":
        n_rows, n_cols = 7001, 2503
        lens = rng.integers(0, 50, n_rows)
        off = np.zeros(n_rows + 1, np.uint32)
        np.cumsum(lens, out=off[1:])
        col = rng.integers(0, n_cols, int(off[-1]), dtype=np.uint32)
        val = rng.uniform(-1, 1, len(col)).astype(dtype)
    else:
        n_rows = n_cols = 40_000
        off, col, val = oracle.gen_powerlaw(7, n_rows, n_cols, dtype)
    lhs = rng.uniform(-1, 1, n_rows).astype(dtype)
    rhs = rng.uniform(-1, 1, n_cols).astype(dtype)
    m = sm.SparseMatCRS.from_raw_parts(n_rows, n_cols, off, col, val)
    ref = float(oracle.mat_inner_prod(off, col, val, lhs, rhs))
    scale = float(oracle.mat_inner_prod(off, col, np.abs(val), np.abs(lhs), np.abs(rhs)))
    tol = (1e-5 if dtype == np.float32 else 1e-12) * scale
    got = m.inner_prod(lhs, rhs)
    assert abs(got - ref) <= tol, (got, ref, scale)
    got_v = m.inner_prod(sm.DenseVec.from_vec(lhs), sm.DenseVec.from_vec(rhs))
    assert got_v == got  # same kernels, deterministic reduction: bitwise reproducible
    for variant in ("stream", "merge", "vector"):
        assert abs(m.inner_prod(lhs, rhs, variant=variant) - ref) <= tol, variant
    # the reference panics (densevec.rs:41) when a vector is too short -- for lhs that means shorter than the last row that
    # holds entries: lhs.get(i) sits inside the entry loop (sparsematrix.rs:165-168)
    last = int(np.nonzero(np.diff(off.astype(np.int64)))[0][-1])
    with pytest.raises(sm.SparseMatPanic) as e:
        m.inner_prod(lhs[:last], rhs)
    assert e.value.status == _lib.SMH_ERR_INDEX_RANGE
    assert "the index is %d" % last in str(e.value)
    with pytest.raises(sm.SparseMatPanic):
        m.inner_prod(lhs, rhs[:int(col.max())])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_matrix_inner_prod_with_trailing_empty_rows_takes_a_short_lhs(gpu, dtype):
    """Only rows with entries index lhs (sparsematrix.rs:165-168): with the last rows empty, an lhs that ends right after
    the last non-empty row is legal in the reference and gives the same sum; one entry shorter panics."""
    rng = np.random.default_rng(11)
    n_rows, n_cols, last = 5000, 3000, 4321
    lens = rng.integers(0, 9, n_rows)
    lens[last] = 5
    lens[last + 1:] = 0
    off = np.zeros(n_rows + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    col = rng.integers(0, n_cols, int(off[-1]), dtype=np.uint32)
    val = rng.uniform(-1, 1, len(col)).astype(dtype)
    lhs = rng.uniform(-1, 1, n_rows).astype(dtype)
    rhs = rng.uniform(-1, 1, n_cols).astype(dtype)
    m = sm.SparseMatCRS.from_raw_parts(n_rows, n_cols, off, col, val)
    ref = float(oracle.mat_inner_prod(off, col, val, lhs, rhs))
    scale = float(oracle.mat_inner_prod(off, col, np.abs(val), np.abs(lhs), np.abs(rhs)))
    tol = (1e-5 if dtype == np.float32 else 1e-12) * scale
    for variant in ("auto", "stream", "merge", "vector"):
        full = m.inner_prod(lhs, rhs, variant=variant)
        short = m.inner_prod(lhs[:last + 1], rhs, variant=variant)
        assert abs(full - ref) <= tol and short == full, variant
    assert m.inner_prod(sm.DenseVec.from_vec(lhs[:last + 1]), sm.DenseVec.from_vec(rhs)) == m.inner_prod(lhs, rhs)
    with pytest.raises(sm.SparseMatPanic) as e:
        m.inner_prod(lhs[:last], rhs)
    assert e.value.status == _lib.SMH_ERR_INDEX_RANGE
