"""Mixed precision on the device (csrc/refine.hip): smh_crs_cast and smh_vec_cast BIT FOR BIT against numpy's astype in both
directions, and the iterative refinement (smh_refine_solve*) BIT FOR BIT against tests/refine_model.py -- x, the outer steps, the inner
solves' bodies in total, rr and the code -- on the cases of tests/refine_cases.py.  The model is fed by the device's own products, each
held to the parity bound first (test_solver_kernels_gpu.device_product): the f64 matrix's by `variant`, the f32 matrix's by `variant_lo`,
a factor pair's through AUTO inside a body and through SEQ at GMRES's cycle end; the factors are the device's own.
tests/test_refine_model.py shows without a GPU that each case moves a bit or a count under every wrong variant that can touch it."""
import ctypes as C
import math

import numpy as np
import pytest

import refine_cases as rc
import refine_model as rm
import sparsemat_amd as sm
from kernel_forms import same
from sparsemat_amd import _lib
from test_gmres_gpu import matrix, status_of
from test_sgs_gpu import is_fused
from test_solver_kernels_gpu import device_product

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
BIG, FIRST_OVER = float(np.finfo(F32).max), float(np.finfo(F32).max) + 2.0 ** 103
# the hand cases of tests/test_refine_model.py, NaN, +-Inf, -0, and three finite values beyond f32's range
SPECIAL = np.array([1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, BIG, np.nextafter(FIRST_OVER, 0.0), FIRST_OVER, -FIRST_OVER, 1e300, 2.0 ** -149, 2.0 ** -150,
                    1.5 * 2.0 ** -149, 2.0 ** -130 * (1 + 2.0 ** -30), -0.0, 0.0, np.inf, -np.inf, np.nan, -1e-310, 1e-46])


def values(nnz, seed=1):
    """nnz f64 values: uniform ones that round in f32, with SPECIAL spread over them (whole, when there is room)"""
    v = np.random.default_rng(seed).uniform(-3, 3, nnz)
    k = min(nnz, len(SPECIAL))
    at = (np.arange(k) * max(1, nnz // max(k, 1))) % max(nnz, 1)
    v[at[:k]] = SPECIAL[:k]
    return v


def ragged(extra, seed=2):
    """rows of 0 .. 130 entries (twice), the last row `extra` entries longer: (n, off, col, val) with nnz mod 4 moving with extra"""
    lens = np.concatenate([np.arange(131), np.arange(131)[::-1]]).astype(np.int64)
    lens[-1] += extra
    n = len(lens)
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    rng = np.random.default_rng(seed)
    col = rng.integers(0, n, int(off[-1])).astype(np.uint32)
    return n, off, col, values(int(off[-1]), seed)


def assert_cast(m, off, col, val, to):
    """m.astype(to) holds numpy's conversion of val, bit for bit, on m's own pattern; its SEQ product is that of a handle made from the
    numpy-cast arrays; the overflow count is numpy's"""
    c = m.astype(to)
    coff, ccol, cval = c.raw_parts()
    want = rm.cast(val, to)
    assert c.dtype == np.dtype(to) and cval.dtype == np.dtype(to)
    assert np.array_equal(coff, off) and np.array_equal(ccol, col)
    bad = np.flatnonzero(~((cval == want) | (np.isnan(cval) & np.isnan(want))))
    assert same(cval, want), (len(bad), bad[:5], cval[bad[:5]], want[bad[:5]])
    assert (c.n_rows(), c.n_cols(), c.orphans()) == (m.n_rows(), m.n_cols(), m.orphans())
    assert c.overflow == (rm.overflow_count(val) if np.dtype(to) == F32 else 0)
    if m.n_rows():
        ref = sm.SparseMatCRS.from_raw_parts(m.n_rows(), m.n_cols(), off, col, want, validate=False)
        x = np.random.default_rng(3).uniform(-1, 1, m.n_cols()).astype(to)
        with np.errstate(all="ignore"):
            assert same(c.mvp(x, variant="seq"), ref.mvp(x, variant="seq"))
    return c


# ---- smh_crs_cast ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1, 2, 3])
def test_crs_cast_on_ragged_rows_at_every_nnz_mod_4(gpu, extra):
    n, off, col, val = ragged(extra)
    assert len(val) % 4 == (len(ragged(0)[3]) + extra) % 4
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    down = assert_cast(m, off, col, val, F32)
    assert down.overflow == 3
    back = assert_cast(down, off, col, rm.cast(val, F32), F64)  # f32 -> f64 is exact
    assert same(rm.cast(back.raw_parts()[2], F32), down.raw_parts()[2])


def test_crs_cast_without_rows_and_with_one_row(gpu):
    empty = sm.SparseMatCRS.from_raw_parts(0, 0, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, F64))
    for to in (F32, F64):
        c = empty.astype(to)
        assert (c.n_rows(), c.n_non_zero_entries(), c.overflow, c.dtype) == (0, 0, 0, np.dtype(to))
    for k in (1, 2, 3, 4, 5, 18):
        val = values(k, seed=k)
        off, col = np.array([0, k], np.uint32), np.arange(k, dtype=np.uint32)
        m = sm.SparseMatCRS.from_raw_parts(1, 18, off, col, val)
        assert_cast(assert_cast(m, off, col, val, F32), off, col, rm.cast(val, F32), F64)


def test_crs_cast_keeps_the_orphan_and_the_settings_and_clones_on_the_same_dtype(gpu):
    orphan = sm.SparseMatCRS.from_triplets([1, 0, 1, 0], [1, 0, 0, 1], np.array([1.0 + 2.0 ** -24, 2.0, 3.0, 1e300]), into_crs=True)
    assert orphan.orphans() == 1
    off, col, val = orphan.raw_parts()
    c = assert_cast(orphan, off, col, val, F32)
    assert c.orphans() == 1
    # a handle without rows but with its orphan (the one-operation replay) continues the replay in the new dtype
    v = 1.0 + 3 * 2.0 ** -24
    first = sm.SparseMatCRS.from_triplets([0], [0], np.array([v]), into_crs=True)
    assert (first.n_rows(), first.orphans()) == (0, 1)
    f32 = first.astype(F32)
    assert (f32.n_rows(), f32.orphans(), f32.dtype) == (0, 1, np.dtype(F32))
    f32.apply([0, 1], [1, 1], np.array([2.0, 3.0], F32))
    whole = sm.SparseMatCRS.from_triplets([0, 0, 1], [0, 1, 1], np.array([v, 2.0, 3.0]).astype(F32), into_crs=True)
    assert all(np.array_equal(p, q) for p, q in zip(f32.raw_parts()[:2], whole.raw_parts()[:2])) and same(f32.raw_parts()[2], whole.raw_parts()[2])
    assert (f32.n_rows(), f32.n_cols(), f32.orphans()) == (whole.n_rows(), whole.n_cols(), whole.orphans())
    # the settings travel as smh_crs_clone copies them; the same dtype IS clone
    n, off, col, val = ragged(1)
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    before = m.resolved_variant()[1]
    m.set_vector_lanes(2)
    assert m.resolved_variant()[1] == 2 != before
    for to in (F32, F64):
        c = m.astype(to)
        assert c.resolved_variant()[1] == m.clone().resolved_variant()[1] == 2
    twin, clone = m.astype(F64), m.clone()
    assert all(np.array_equal(p, q) for p, q in zip(twin.raw_parts()[:2], clone.raw_parts()[:2])) and same(twin.raw_parts()[2], clone.raw_parts()[2])
    assert twin.overflow == 0 and twin._h.value != m._h.value


def test_crs_cast_statuses_and_borrowed_arrays(gpu):
    L = sm.lib()
    n, off, col, val = ragged(0)
    m = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    h, over = C.c_void_p(), C.c_size_t()
    assert L.smh_crs_cast(None, _lib.SMH_F32, C.byref(h), C.byref(over)) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_cast(m._h, _lib.SMH_F32, None, C.byref(over)) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_cast(m._h, 2, C.byref(h), C.byref(over)) == _lib.SMH_ERR_INVALID and not h.value
    assert L.smh_crs_cast(m._h, _lib.SMH_F32, C.byref(h), None) == 0 and h.value  # (overflow_out is optional)
    L.smh_crs_destroy(h)
    # a borrowed handle works on the caller's arrays: smh_crs_create_dev takes 16-byte aligned value arrays only, so a start 4 or 8
    # bytes past a 16-byte boundary reaches the conversion through smh_vec_cast (below: the same kernel); a borrowed aligned one here
    import torch
    t_off, t_col = torch.from_numpy(off.astype(np.int32)).cuda(), torch.from_numpy(col.astype(np.int32)).cuda()
    t_val = torch.from_numpy(val).cuda()
    b = sm.SparseMatCRS.from_device_parts(n, n, len(val), t_off.data_ptr(), t_col.data_ptr(), t_val.data_ptr(), F64, keep=(t_off, t_col, t_val))
    assert_cast(b, off, col, val, F32)
    assert status_of(lambda: sm.SparseMatCRS.from_device_parts(n, n, len(val) - 1, t_off.data_ptr(), t_col.data_ptr(), t_val.data_ptr() + 8, F64))[0] == _lib.SMH_ERR_INVALID


# ---- smh_vec_cast ------------------------------------------------------------------------------------------------------------------------
GRID_SPAN = 4 * 256 * 512  # elements one trip of the conversion's grid covers


def wrapped(base, skip_bytes, n, dtype):
    """n elements of `dtype` inside the DenseVec base, starting skip_bytes past its (256-byte aligned) start"""
    return sm.DenseVec.from_device_ptr(base.data_ptr() + skip_bytes, n, dtype, keep=base)


@pytest.mark.parametrize("n", list(range(6)) + list(range(257, 265)) + [GRID_SPAN + 7])
def test_vec_cast_bits(gpu, n):
    v = values(n, seed=n % 11)
    d = sm.DenseVec.from_vec(v)
    down = d.astype(F32)
    assert down.dtype == np.dtype(F32) and same(down.to_numpy(), rm.cast(v, F32))
    up = down.astype(F64)
    assert same(up.to_numpy(), rm.cast(rm.cast(v, F32), F64))
    assert same(d.astype(F64).to_numpy(), v) and same(d.to_numpy(), v)  # (the same dtype: a copy; the source is read only)


@pytest.mark.parametrize("src_skip, dst_skip", [(0, 4), (0, 8), (0, 12), (8, 0), (8, 4), (8, 8), (8, 12)])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 262])
def test_vec_cast_from_and_to_arrays_that_start_off_a_16_byte_boundary(gpu, n, src_skip, dst_skip):
    """the f64 array 0 or 8 bytes, the f32 array 0, 4, 8 or 12 bytes past a 16-byte boundary, in both directions: the head runs to the
    f32 array's boundary and the groups of four are taken when the f64 array is aligned there too"""
    L = sm.lib()
    v = values(n, seed=5)
    wide, narrow = sm.DenseVec.zeros(n + 8, F64), sm.DenseVec.zeros(n + 8, F32)
    assert wide.data_ptr() % 16 == 0 and narrow.data_ptr() % 16 == 0
    src, dst = wrapped(wide, src_skip, n, F64), wrapped(narrow, dst_skip, n, F32)
    assert L.smh_vec_upload(src._h, v.ctypes.data if n else None) == 0
    assert L.smh_vec_cast(src._h, dst._h) == 0
    assert same(dst.to_numpy(), rm.cast(v, F32))
    guard = narrow.to_numpy()
    assert not guard[:dst_skip // 4].any() and not guard[dst_skip // 4 + n:].any()  # (nothing written beside the n elements)
    wide2 = sm.DenseVec.zeros(n + 8, F64)
    back = wrapped(wide2, src_skip, n, F64)
    assert L.smh_vec_cast(dst._h, back._h) == 0
    assert same(back.to_numpy(), rm.cast(rm.cast(v, F32), F64))
    guard = wide2.to_numpy()
    assert not guard[:src_skip // 8].any() and not guard[src_skip // 8 + n:].any()


def test_vec_cast_statuses(gpu):
    L = sm.lib()
    a, b, c = sm.DenseVec.from_vec(np.ones(8)), sm.DenseVec.zeros(8, F32), sm.DenseVec.zeros(7, F32)
    assert L.smh_vec_cast(None, b._h) == L.smh_vec_cast(a._h, None) == _lib.SMH_ERR_INVALID
    assert L.smh_vec_cast(a._h, c._h) == _lib.SMH_ERR_DIM_MISMATCH
    alias = sm.DenseVec.from_device_ptr(a.data_ptr(), 8, F32, keep=a)
    inside = sm.DenseVec.from_device_ptr(a.data_ptr() + 32, 8, F32, keep=a)
    assert L.smh_vec_cast(a._h, alias._h) == L.smh_vec_cast(a._h, inside._h) == L.smh_vec_cast(alias._h, a._h) == _lib.SMH_ERR_INVALID
    assert b"share storage" in L.smh_last_error()
    assert a.to_numpy().tolist() == [1.0] * 8


# ---- the refinement ----------------------------------------------------------------------------------------------------------------------
class Device:
    """A case on the device: the f64 handle, its f32 copy (the library's own cast, pinned to numpy's), the device's own factors, and the
    model fed by the device's checked products."""

    def __init__(self, case, variant="seq", variant_lo="seq"):
        self.case, self.variant, self.variant_lo = case, variant, variant_lo
        self.off, self.col, self.val, self.b, self.x0 = case.system()
        self.a = matrix(self.off, self.col, self.val)
        self.a_lo = self.a.astype(F32)
        self.val32 = rm.cast(self.val, F32)
        assert same(self.a_lo.raw_parts()[2], self.val32) and self.a_lo.overflow == 0
        handles = {id(self.val32): self.a_lo}
        self.factor, self.parts = None, None
        if case.precond == "ilu":
            self.factor, zero_pivot = self.a_lo.ilu0()
            assert zero_pivot is None
            self.parts = self.factor.raw_parts()
            handles[id(self.parts[2])] = self.factor
        elif case.precond == "fsai":
            g, gt, bad = self.a_lo.fsai() if case.inner == "cg" else self.a_lo.fsai_ns()
            assert bad is None
            self.factor = (g, gt)
            self.parts = (g.raw_parts(), gt.raw_parts())
            handles[id(self.parts[0][2])], handles[id(self.parts[1][2])] = g, gt

        def product(off, col, val, kind):
            return device_product(handles[id(val)], {"matrix": variant_lo, "body": "auto", "end": "seq"}[kind], off, col, val)
        if case.name == "nan_b":  # (NaN data: the oracle's product, which SEQ's equals bit for bit, without the parity bound)
            assert variant == variant_lo == "seq"
            product = rc.oracle_products
        self.inner = case.inner_of(self.off, self.col, self.val32, self.parts, product, fused=case.inner == "cg" and is_fused(self.a_lo, variant_lo))
        self.product = product(self.off, self.col, self.val, "matrix") if case.name == "nan_b" else device_product(self.a, variant, self.off, self.col, self.val)

    def model(self):
        return rm.refine(self.product, self.inner, self.b, self.x0, self.case.tol, self.case.outer_max)

    def solver(self, check_every=0):
        c = self.case
        return sm.IterativeRefinement(c.tol, c.outer_max, c.inner, c.precond, c.inner_tol, c.inner_iter_max, c.restart, self.variant, self.variant_lo,
                                      check_every)

    def host(self, check_every=0):
        s, x = self.solver(check_every), self.x0.copy()
        s.solve(self.a, self.b, x, mat_lo=self.a_lo, factor=self.factor)
        return x, s.outer_iterations, s.iterations, s.r_norm_squared, s.code

    def vec(self, check_every=0):
        s = self.solver(check_every)
        bd, xd = sm.DenseVec.from_vec(self.b), sm.DenseVec.from_vec(self.x0)
        s.solve(self.a, bd, xd, mat_lo=self.a_lo, factor=self.factor)
        assert same(bd.to_numpy(), self.b)  # (b is read only)
        return xd.to_numpy(), s.outer_iterations, s.iterations, s.r_norm_squared, s.code


def assert_result(got, want, what):
    x, outer, iters, rr, code = got
    assert outer == want.outer, (what, "outer", outer, want.outer)
    assert iters == want.iterations, (what, "inner bodies", iters, want.iterations, want.inner_list)
    assert code == want.code, (what, "code", code, want.code)
    assert same(F64(rr), F64(want.rr)), (what, "r.r", rr, want.rr)
    bad = np.flatnonzero(~((x == want.x) | (np.isnan(x) & np.isnan(want.x))))
    assert same(x, want.x), (what, "x", len(bad), bad[:5], x[bad[:5]], want.x[bad[:5]])


def true_residual(d, x):
    r = d.b.astype(np.longdouble) - d.product(x).astype(np.longdouble)
    return float(np.sqrt(np.sum(r * r)))


@pytest.mark.parametrize("case", rc.CASES, ids=[c.name for c in rc.CASES])
def test_cases_equal_the_model_fed_by_the_checked_device_products(gpu, case):
    d = Device(case)
    want = d.model()
    assert want.code == case.code
    assert_result(d.vec(), want, (case.name, "vec"))
    assert_result(d.host(), want, (case.name, "host"))
    if case.code == 0 and case.tol < 1.0 and case.n:
        assert true_residual(d, want.x) < 2 * case.tol  # (the true residual, from numpy)
    if case.name in ("stall", "nan_b"):
        assert same(want.x, d.x0) == (case.name == "nan_b")  # NaN: x0 comes back; a stall: the better iterate


@pytest.mark.parametrize("name", ["tridiag259", "gmres5", "bicgstab+fsai"])
def test_check_every_changes_no_bit(gpu, name):
    d = Device(rc.BY_NAME[name])
    want = d.model()
    for ce in (1, 8):
        assert_result(d.vec(ce), want, (name, "check_every", ce))
        assert_result(d.host(ce), want, (name, "check_every, host", ce))


@pytest.mark.parametrize("variant_lo", ["stream", "seq", "auto"])
@pytest.mark.parametrize("variant", ["stream", "seq", "auto"])
def test_stream_seq_and_auto_products_on_both_handles(gpu, variant, variant_lo):
    d = Device(rc.BY_NAME["tridiag261"], variant, variant_lo)
    assert_result(d.vec(), d.model(), (variant, variant_lo))


def test_python_class_casts_and_factors_by_itself(gpu):
    """mat_lo=None casts, factor=None factors the cast matrix (ilu0; fsai for CG, fsai_ns otherwise): the bits of the passed ones"""
    for name in ("cg+ilu", "cg+fsai", "bicgstab+fsai", "gmres30+ilu", "tridiag258"):
        d = Device(rc.BY_NAME[name])
        want = d.model()
        s, x = d.solver(), d.x0.copy()
        s.solve(d.a, d.b, x)
        assert_result((x, s.outer_iterations, s.iterations, s.r_norm_squared, s.code), want, (name, "by itself"))
        assert s.mat_lo.dtype == np.dtype(F32) and same(s.mat_lo.raw_parts()[2], d.val32)
        if d.case.precond == "ilu":
            assert same(s.factor.raw_parts()[2], d.parts[2])
        elif d.case.precond == "fsai":
            assert same(s.factor[0].raw_parts()[2], d.parts[0][2]) and same(s.factor[1].raw_parts()[2], d.parts[1][2])
        else:
            assert s.factor is None


def test_two_runs_give_the_same_result(gpu):
    for name in ("cg+sgs", "gmres30+ilu", "tridiag2051"):
        d = Device(rc.BY_NAME[name], "auto", "auto")
        first = d.vec()
        for ce in (0, 3):
            again = d.vec(ce)
            assert same(again[0], first[0]) and again[1:] == first[1:], name


def test_statuses_leave_x_untouched(gpu):
    L = sm.lib()
    d = Device(rc.BY_NAME["gmres30+ilu"])
    n = 576
    a, a_lo, f = d.a, d.a_lo, d.factor
    b, x = np.ones(n), np.full(n, 7.0)
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x)
    b32, x32 = sm.DenseVec.from_vec(b.astype(F32)), sm.DenseVec.from_vec(x.astype(F32))
    short = sm.DenseVec.from_vec(np.ones(n - 1))
    small = matrix(*rc.tridiag(100)[:3])
    small_lo = small.astype(F32)
    rect = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 1], np.ones(2))
    rect_lo = rect.astype(F32)
    INV, DIM, SQ = _lib.SMH_ERR_INVALID, _lib.SMH_ERR_DIM_MISMATCH, _lib.SMH_ERR_NOT_SQUARE
    CG, BI, GM = _lib.SMH_INNER_CG, _lib.SMH_INNER_BICGSTAB, _lib.SMH_INNER_GMRES
    NONE, JAC, SGS, ILU, FSAI = 0, 1, 2, 3, 4

    def vec(a_, lo_, inner, precond, f1, f2, b_, x_, restart=0):
        h = lambda o: o._h if o is not None else None
        return L.smh_refine_solve_vec(h(a_), h(lo_), inner, precond, h(f1), h(f2), h(b_), h(x_), 1e-9, 0, 0.0, 0, restart, 0, 0, 0, None, None, None, None)

    def host(a_, lo_, inner, precond, f1, f2, b_, x_, restart=0):
        h = lambda o: o._h if o is not None else None
        return L.smh_refine_solve(h(a_), h(lo_), inner, precond, h(f1), h(f2), b_.ctypes.data if b_ is not None else None, len(b_) if b_ is not None else n,
                                  x_.ctypes.data if x_ is not None else None, len(x_) if x_ is not None else n, 1e-9, 0, 0.0, 0, restart, 0, 0, 0, None, None, None,
                                  None)

    # NULL handles and vectors
    assert vec(None, a_lo, CG, NONE, None, None, bd, xd) == vec(a, None, CG, NONE, None, None, bd, xd) == INV
    assert vec(a, a_lo, CG, NONE, None, None, None, xd) == vec(a, a_lo, CG, NONE, None, None, bd, None) == INV
    assert host(None, a_lo, CG, NONE, None, None, b, x) == host(a, None, CG, NONE, None, None, b, x) == INV
    assert host(a, a_lo, CG, NONE, None, None, None, x) == host(a, a_lo, CG, NONE, None, None, b, None) == INV
    # the dtypes: a f64, a_lo f32, the vectors f64
    assert vec(a_lo, a_lo, CG, NONE, None, None, bd, xd) == vec(a, a, CG, NONE, None, None, bd, xd) == INV
    assert host(a_lo, a_lo, CG, NONE, None, None, b, x) == host(a, a, CG, NONE, None, None, b, x) == INV
    assert vec(a, a_lo, CG, NONE, None, None, b32, xd) == vec(a, a_lo, CG, NONE, None, None, bd, x32) == INV
    # b and x in one storage
    assert vec(a, a_lo, CG, NONE, None, None, xd, xd) == host(a, a_lo, CG, NONE, None, None, x, x) == INV
    for call, fb, fx in ((vec, bd, xd), (host, b, x)):
        # an unknown inner or precond; CG with Jacobi
        assert call(a, a_lo, 3, NONE, None, None, fb, fx) == call(a, a_lo, -1, NONE, None, None, fb, fx) == INV
        assert call(a, a_lo, GM, 5, None, None, fb, fx) == call(a, a_lo, GM, -1, None, None, fb, fx) == INV
        assert call(a, a_lo, CG, JAC, None, None, fb, fx) == INV
        assert b"no device-vector form" in L.smh_last_error()
        # a factor given where the kind takes none, missing where it takes one
        assert call(a, a_lo, GM, NONE, f, None, fb, fx) == call(a, a_lo, GM, SGS, f, None, fb, fx) == call(a, a_lo, BI, JAC, None, f, fb, fx) == INV
        assert call(a, a_lo, GM, ILU, None, None, fb, fx) == call(a, a_lo, GM, ILU, f, f, fb, fx) == INV
        assert call(a, a_lo, GM, FSAI, f, None, fb, fx) == call(a, a_lo, GM, FSAI, None, f, fb, fx) == call(a, a_lo, CG, FSAI, None, None, fb, fx) == INV
        # a_lo's dims; not square; restart
        assert call(a, small_lo, CG, NONE, None, None, fb, fx) == DIM
        assert call(rect, rect_lo, CG, NONE, None, None, fb, fx) == SQ
        assert call(a, a_lo, GM, NONE, None, None, fb, fx, restart=129) == INV
        assert b"restart" in L.smh_last_error()
    # the vectors' dims
    assert vec(a, a_lo, CG, NONE, None, None, short, xd) == vec(a, a_lo, CG, NONE, None, None, bd, short) == DIM
    assert host(a, a_lo, CG, NONE, None, None, b[:-1], x) == host(a, a_lo, CG, NONE, None, None, b, x[:-1]) == DIM
    # what the inner entry point refuses about a_lo and the factors comes back with its own code: a factor of another dimension
    small_f = small_lo.ilu0()[0]
    assert vec(a, a_lo, GM, ILU, small_f, None, bd, xd) == host(a, a_lo, GM, ILU, small_f, None, b, x) == DIM
    assert vec(a, a_lo, CG, ILU, small_f, None, bd, xd) == DIM
    f64_factor = a.ilu0()[0]
    assert vec(a, a_lo, BI, ILU, f64_factor, None, bd, xd) == INV
    assert x.tolist() == [7.0] * n and xd.to_numpy().tolist() == [7.0] * n
    # the Python class reports nothing after a refusal
    s = sm.IterativeRefinement(1e-9, inner="cg", precond="jacobi")
    assert status_of(lambda: s.solve(a, bd, xd, mat_lo=a_lo))[0] == INV and s.iterations is None and s.code is None
    # ... and the output pointers may be NULL: the defaults solve the system
    assert vec(a, a_lo, GM, ILU, f, None, bd, xd, restart=0) == 0
    got = xd.to_numpy()
    assert float(np.linalg.norm(b - d.product(got))) < 2e-9
