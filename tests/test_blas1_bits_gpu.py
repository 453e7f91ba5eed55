"""The DenseVec kernels (K3 / K4, blas1.hip) through their public entry points -- smh_vec_add / sub / scale / axpy / xpby / dot /
norm_squared / norm, the DenseVec operators and smh_blas_dot_dev / axpy_dev / xpby_dev -- bit for bit against tests/blas1_model.py, in
f32 and f64.  NaN is compared by class (kernel_forms.same); everything else is bit equality.

The operands live inside larger device buffers (torch tensors, wrapped with DenseVec.from_device_ptr at an element offset): NaN
around a reduction's operands, a sentinel around an element-wise operation's, and every byte that an operation may not touch is
compared afterwards.  The cases are tests/blas1_cases.py's; tests/test_blas1_model.py shows on the CPU which wrong kernel each of
them would catch."""
import ctypes as C
import math

import numpy as np
import pytest

import blas1_cases as bc
import blas1_model as bm
import sparsemat_amd as sm
from kernel_forms import same
from sparsemat_amd import _lib
from sparsemat_amd._lib import check, lib

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
BOTH = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
PAD = 8  # entries in front of and behind every operand: 32 / 64 bytes, so an element offset of 0 stays 16-byte aligned
RED = {dt: {c.name: c for c in bc.reduction_cases(dt)} for dt in bc.DTYPES}
EW = {dt: {c.name: c for c in bc.ew_cases(dt)} for dt in bc.DTYPES}


def by_group(cases, pick):
    return [pytest.param(dt, name, id="%s-%s" % (np.dtype(dt).name, name)) for dt in bc.DTYPES for name, c in cases[dt].items() if pick(c)]


class Buf:
    """[PAD x fill][off x fill][values][extra x fill][PAD x fill] on the device; the operand is the window of `values`"""

    def __init__(self, values, off=0, fill=np.nan, extra=0):
        import torch
        values = np.ascontiguousarray(values)
        self.dtype, self.n, self.lo = values.dtype, len(values), PAD + off
        self.host = np.full(self.lo + self.n + extra + PAD, fill, self.dtype)
        self.host[self.lo:self.lo + self.n] = values
        self.t = torch.from_numpy(self.host.copy()).cuda()
        assert self.t.data_ptr() % 16 == 0

    def ptr(self, start=0):
        return self.t.data_ptr() + (self.lo + start) * self.dtype.itemsize

    def vec(self, n=None, start=0):
        return sm.DenseVec.from_device_ptr(self.ptr(start), self.n - start if n is None else n, self.dtype.type, keep=self.t)

    def read(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy()

    def window(self):
        return self.read()[self.lo:self.lo + self.n]

    def assert_untouched(self, what=""):
        assert self.read().tobytes() == self.host.tobytes(), what

    def assert_window(self, want, touched, what=""):
        """the first `touched` entries of the window are `want`'s (NaN by class), every other byte of the buffer is as it was"""
        got, full = self.read(), self.host.copy()
        a, b = self.lo, self.lo + touched
        assert same(got[a:b], want[:touched]), what
        assert want[touched:].tobytes() == self.host[b:self.lo + self.n].tobytes(), what   # (the model agrees about the rest)
        full[a:b] = got[a:b]
        assert got.tobytes() == full.tobytes(), what


def status_of(call, *args):
    with pytest.raises(sm.SparseMatPanic) as e:
        check(call(*args))
    return e.value.status, str(e.value)


# ---- reductions ------------------------------------------------------------------------------------------------------------------
def place(case, dtype):
    """(x, y, X, Y, xv, yv): the case's arrays, their device buffers and the wrapped windows"""
    x, y = case.arrays(dtype)
    if case.shared:   # two windows of one buffer, y `shift` entries behind x
        shift = case.off_y - case.off_x
        X = Y = Buf(np.concatenate([x[:shift], y]), case.off_x)
        assert np.array_equal(X.host[X.lo:X.lo + len(x)], x)
        return x, y, X, Y, X.vec(len(x)), X.vec(len(y), start=shift)
    X, Y = Buf(x, case.off_x), Buf(y, case.off_y)
    return x, y, X, Y, X.vec(), Y.vec()


def check_reduction(case, dtype):
    x, y, X, Y, xv, yv = place(case, dtype)
    aligned = case.aligned(dtype)
    assert aligned == (xv.data_ptr() % 16 == 0 and yv.data_ptr() % 16 == 0)
    want = bm.dot(x, y, aligned)
    got = xv.inner_prod(yv)
    assert type(got) is dtype and same(got, want), (case.name, got, want)
    assert same(yv.inner_prod(xv), bm.dot(y, x, aligned)), case.name
    assert same(xv * yv, want) and same(xv.inner_prod(yv), got), case.name            # the `v * w` sugar; reproducible
    for v, h, off in ((xv, x, case.off_x), (yv, y, case.off_y)):
        alone = bc.is_aligned(dtype, off)
        nn = v.norm_squared()
        assert type(nn) is dtype and same(nn, bm.norm_squared(h, alone)), (case.name, nn)
        assert same(np.float64(v.norm()), np.float64(bm.norm(h, alone))), case.name
    X.assert_untouched(case.name)
    Y.assert_untouched(case.name)
    return got


@pytest.mark.parametrize("dtype,name", by_group(RED, lambda c: c.group == "size"))
def test_reduction_sizes(gpu, dtype, name):
    check_reduction(RED[dtype][name], dtype)


@BOTH
@pytest.mark.parametrize("n", bc.ALIGN_SIZES)
def test_reduction_alignment(gpu, dtype, n):
    """x only, y only, both off a 16-byte boundary: V = 1; both one whole vector further: V again"""
    x, y = bc.data(n, dtype, bc.SEED_X), bc.data(n, dtype, bc.SEED_Y)
    assert not same(bm.dot(x, y, True), bm.dot(x, y, False))    # this size can tell the two paths apart
    cases = [c for c in RED[dtype].values() if c.group == "align" and c.name.startswith("n%d-" % n)]
    assert len(cases) == len(bc.offset_pairs(dtype)) and any(c.aligned(dtype) for c in cases)
    for case in cases:
        check_reduction(case, dtype)


@BOTH
def test_reduction_truncation_and_read_only_overlap(gpu, dtype):
    """the shorter operand decides, the NaN behind it never reaches the sum; two windows of one buffer may overlap in a dot"""
    cases = [c for c in RED[dtype].values() if c.group in ("trunc", "overlap")]
    assert len(cases) == 6
    for case in cases:
        got = check_reduction(case, dtype)
        assert np.isfinite(got), case.name
    n = 2049
    B = Buf(bc.data(n, dtype, 22))
    one, two = B.vec(), B.vec()       # distinct handles on one pointer: the single-read path of norm_squared, reached through dot
    assert one.data_ptr() == two.data_ptr()
    assert same(one.inner_prod(two), one.norm_squared()) and same(one.inner_prod(two), bm.norm_squared(bc.data(n, dtype, 22)))
    B.assert_untouched()


@BOTH
def test_reduction_special_values(gpu, dtype):
    """one NaN / Inf anywhere -- a vector of the body, the n % V tail, the last thread's share, the second workgroup --, Inf - Inf,
    Inf * 0, overflow of the sum, products that are all -0 (the accumulators start at +0: +0), products that are all subnormal"""
    seen = set()
    for case in RED[dtype].values():
        if case.group != "special":
            continue
        got = check_reduction(case, dtype)
        kind = case.name.split("-n")[0]
        seen.add(kind)
        if kind in ("nan", "inf-inf", "inf*0"):
            assert np.isnan(got), case.name
        elif kind in ("+inf", "overflow", "-inf"):
            assert np.isinf(got) and (got < 0) == (kind == "-inf"), case.name
        elif kind == "minus-zeros":
            assert got == 0 and not np.signbit(got), case.name
        else:
            assert kind == "subnormal-products" and got != 0 and np.isfinite(got), case.name
    assert len(seen) == 8


# ---- element-wise ----------------------------------------------------------------------------------------------------------------
def ew_operations(a):
    """(name, the call on the two DenseVecs, the model on the two host arrays, does it touch all of x)"""
    return [
        ("add", lambda xv, yv: xv.add(yv), lambda x, y: bm.add(x, y), False),
        ("sub", lambda xv, yv: xv.sub(yv), lambda x, y: bm.sub(x, y), False),
        ("scale", lambda xv, yv: xv.scale(a), lambda x, y: bm.scale(x, a), True),
        ("axpy", lambda xv, yv: xv.axpy(a, yv), lambda x, y: bm.axpy(x, a, y), False),
        ("xpby", lambda xv, yv: xv.xpby(a, yv), lambda x, y: bm.xpby(x, a, y), False),
        ("+=", lambda xv, yv: xv.__iadd__(yv), lambda x, y: bm.add(x, y), False),
        ("-=", lambda xv, yv: xv.__isub__(yv), lambda x, y: bm.sub(x, y), False),
        ("*=", lambda xv, yv: xv.__imul__(a), lambda x, y: bm.scale(x, a), True),
    ]


def check_elementwise(x, y, off_x, off_y, a, what, operators=True):
    s = bc.sentinel(x.dtype)
    for name, call, model, all_of_x in ew_operations(a):
        # (behind y as many sentinels as x is longer: a sweep that ran on would read them, not another allocation)
        X, Y = Buf(x, off_x, s), Buf(y, off_y, s, extra=len(x) - len(y))
        call(X.vec(), Y.vec())
        X.assert_window(model(x, y), len(x) if all_of_x else len(y), (what, name))
        Y.assert_untouched((what, name))
    if operators and len(x) == len(y):
        X, Y = Buf(x, off_x, s), Buf(y, off_y, s)
        xv, yv = X.vec(), Y.vec()
        assert same((xv + yv).to_numpy(), bm.add(x, y)) and same((xv - yv).to_numpy(), bm.sub(x, y)), what
        assert same((xv * a).to_numpy(), bm.scale(x, a)), what
        X.assert_untouched(what)
        Y.assert_untouched(what)


@pytest.mark.parametrize("dtype,name", by_group(EW, lambda c: c.off_x == c.off_y == 0 and c.n_x == c.n_y))
def test_elementwise_sizes(gpu, dtype, name):
    """the small sizes, then the vector path's grid at its cap, one element beyond, and in its second trip"""
    case = EW[dtype][name]
    x, y = case.arrays(dtype)
    check_elementwise(x, y, 0, 0, bc.EW_SCALAR, name)


@BOTH
@pytest.mark.parametrize("n", bc.EW_UNALIGNED_SIZES + (5, 257))
def test_elementwise_alignment(gpu, dtype, n):
    """x only, y only, both off a 16-byte boundary (the VEC = false kernel, its grid at the cap and beyond), both a vector further"""
    cases = [c for c in EW[dtype].values() if c.n_x == n and c.name.startswith("n%d-off" % n)]
    assert len(cases) == len(bc.offset_pairs(dtype))
    for case in cases:
        x, y = case.arrays(dtype)
        check_elementwise(x, y, case.off_x, case.off_y, bc.EW_SCALAR, case.name, operators=False)


@BOTH
def test_elementwise_shorter_rhs_leaves_the_rest_alone(gpu, dtype):
    """x[len(y):] stays as it was, with len(y) % V != 0, on both paths; so does everything in front of and behind the vectors"""
    cases = [c for c in EW[dtype].values() if c.n_y < c.n_x]
    assert len(cases) == 5 and any(c.n_y % bc.vec_len(dtype) and not bc.is_aligned(dtype, c.off_x, c.off_y) for c in cases)
    for case in cases:
        x, y = case.arrays(dtype)
        check_elementwise(x, y, case.off_x, case.off_y, bc.EW_SCALAR, case.name)


@BOTH
def test_scalars_are_rounded_once(gpu, dtype):
    """the API's double reaches the kernel as T(a): 0.1 and 1/3 (not representable), 1 + 2^-24 + 2^-50 (rounded twice it would be 1
    in f32), the signed zeros, 1e39 (+Inf in f32), 1e-46 (+0 in f32), NaN"""
    n = bc.SCALAR_SIZE
    x, y = bc.data(n, dtype, 43), bc.data(n, dtype, 44)
    for a in bc.SCALARS:
        for off in ((0, 0), (1, 0)):
            check_elementwise(x, y, off[0], off[1], a, ("scalar", a, off), operators=False)


@BOTH
def test_full_aliasing_is_legal(gpu, dtype):
    """x.add(x), x.sub(x) (+0 everywhere, NaN where x is not finite), x.axpy(a, x), x.xpby(b, x): one handle, and two handles on one
    pointer -- each the model applied to a copy"""
    x = np.concatenate([bc.data(1027, dtype, 45), bc.special_pool(dtype)])
    a, s = bc.EW_SCALAR, bc.sentinel(dtype)
    ops = [("add", lambda v, w: v.add(w), lambda h: bm.add(h, h.copy())), ("sub", lambda v, w: v.sub(w), lambda h: bm.sub(h, h.copy())),
           ("axpy", lambda v, w: v.axpy(a, w), lambda h: bm.axpy(h, a, h.copy())), ("xpby", lambda v, w: v.xpby(a, w), lambda h: bm.xpby(h, a, h.copy()))]
    for name, call, model in ops:
        for off in (0, 1):
            for two_handles in (False, True):
                X = Buf(x, off, s)
                v = X.vec()
                call(v, X.vec() if two_handles else v)
                X.assert_window(model(x), len(x), (name, off, two_handles))
    z = bm.sub(x, x.copy())
    assert np.array_equal(np.isnan(z), ~np.isfinite(x)) and not np.signbit(z[np.isfinite(x)]).any() and (z[np.isfinite(x)] == 0).all()


@BOTH
def test_elementwise_special_values(gpu, dtype):
    """every pairing of +-0, +-Inf, NaN, the largest finite, the smallest normal, subnormals and ordinary numbers, with scalars that
    take products into the subnormals, to zero and over the top: numpy's bits; gradual underflow is kept"""
    x, y = bc.special_pairs(dtype)
    tiny = np.finfo(dtype).tiny
    want = bm.axpy(x, float(tiny), y)
    assert ((want != 0) & (np.abs(want) < tiny)).any()      # (a flushed subnormal would be seen)
    for a in bc.special_scalars(dtype):
        for off in ((0, 0), (1, 1)):
            check_elementwise(x, y, off[0], off[1], a, ("special", a, off), operators=False)


# ---- the entry points on raw pointers with device-resident scalars ---------------------------------------------------------------
def code(dtype):
    return _lib.dtype_code(np.dtype(dtype))


@BOTH
def test_dev_entry_points_match_the_host_scalar_forms(gpu, dtype):
    """smh_blas_axpy_dev / xpby_dev / dot_dev on a non-default stream, scalar and result in device memory: the bits of the DenseVec
    forms and of the model, with an unaligned x or y, a result that is not the library's scratch, and a scratch of exactly
    smh_blas_dot_scratch_bytes() whose neighbours survive"""
    import torch
    n, s = 4101, bc.sentinel(dtype)
    x, y = bc.data(n, dtype, 46), bc.data(n, dtype, 47)
    a = bm.scalar(bc.SCALARS[1], dtype)                     # 1/3 as a T
    side = torch.cuda.Stream()
    stream = C.c_void_p(side.cuda_stream)
    need = lib().smh_blas_dot_scratch_bytes()
    for ox, oy in ((0, 0), (1, 0), (0, 1), (bc.vec_len(dtype), bc.vec_len(dtype))):
        for fn, model, method in ((lib().smh_blas_axpy_dev, bm.axpy, "axpy"), (lib().smh_blas_xpby_dev, bm.xpby, "xpby")):
            X, Y, A = Buf(x, ox, s), Buf(y, oy, s), Buf(np.array([a], dtype), 0, s)
            torch.cuda.synchronize()
            check(fn(code(dtype), C.c_void_p(X.ptr()), C.c_void_p(A.ptr()), C.c_void_p(Y.ptr()), n, stream))
            side.synchronize()
            want = model(x, a, y)
            X.assert_window(want, n, (method, ox, oy))
            Y.assert_untouched()
            A.assert_untouched()
            H = Buf(x, ox, s)                               # the host-scalar form: float(a) is rounded back to the same T
            getattr(H.vec(), method)(float(a), Y.vec())
            assert same(H.window(), X.window())
        X, Y, R = Buf(x, ox), Buf(y, oy), Buf(np.array([s], dtype), 0, s)
        guard = 64
        scratch = torch.full((guard + need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        assert scratch.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        check(lib().smh_blas_dot_dev(code(dtype), C.c_void_p(X.ptr()), C.c_void_p(Y.ptr()), n, C.c_void_p(R.ptr()),
                                     C.c_void_p(scratch.data_ptr() + guard), stream))
        side.synchronize()
        want = bm.dot(x, y, bc.is_aligned(dtype, ox, oy))
        R.assert_window(np.array([want], dtype), 1, ("dot", ox, oy))
        assert same(X.vec().inner_prod(Y.vec()), want)
        around = scratch.cpu().numpy()
        assert (around[:guard] == 0xA5).all() and (around[guard + need:] == 0xA5).all()
        X.assert_untouched()
        Y.assert_untouched()


@BOTH
def test_vec_norm_is_the_double_sqrt_of_the_widened_norm_squared(gpu, dtype):
    for n in (0, 1, 5, 2049):
        x = bc.data(n, dtype, 48)
        v = Buf(x).vec()
        nn, nrm = C.c_double(-1.0), C.c_double(-1.0)
        check(lib().smh_vec_norm_squared(v._h, C.byref(nn)))
        check(lib().smh_vec_norm(v._h, C.byref(nrm)))
        assert nn.value == float(bm.norm_squared(x)) and nrm.value == math.sqrt(nn.value) == bm.norm(x)
        assert same(np.float64(nn.value), np.float64(bm.norm_squared(x)))


# ---- statuses --------------------------------------------------------------------------------------------------------------------
def test_statuses_of_the_vector_entry_points(gpu):
    L, INVALID, DIM = lib(), _lib.SMH_ERR_INVALID, _lib.SMH_ERR_DIM_MISMATCH
    a, b, short = sm.DenseVec.from_vec(np.ones(8, F32)), sm.DenseVec.from_vec(np.ones(8, F64)), sm.DenseVec.from_vec(np.ones(5, F32))
    out = C.c_double(7.0)
    for fn in (L.smh_vec_add, L.smh_vec_sub):
        assert status_of(fn, None, a._h)[0] == status_of(fn, a._h, None)[0] == INVALID
        assert status_of(fn, a._h, b._h) == (INVALID, "vector dtype mismatch")
        assert status_of(fn, short._h, a._h) == (DIM, "Dimension mismatch")
    for fn in (L.smh_vec_axpy, L.smh_vec_xpby):
        assert status_of(fn, None, 1.0, a._h)[0] == status_of(fn, a._h, 1.0, None)[0] == INVALID
        assert status_of(fn, a._h, 1.0, b._h)[0] == INVALID and status_of(fn, short._h, 1.0, a._h)[0] == DIM
    assert status_of(L.smh_vec_scale, None, 1.0)[0] == INVALID
    assert status_of(L.smh_vec_dot, None, a._h, C.byref(out))[0] == status_of(L.smh_vec_dot, a._h, None, C.byref(out))[0] == INVALID
    assert status_of(L.smh_vec_dot, a._h, b._h, C.byref(out))[0] == status_of(L.smh_vec_dot, a._h, a._h, None)[0] == INVALID
    assert status_of(L.smh_vec_norm_squared, None, C.byref(out))[0] == status_of(L.smh_vec_norm, None, C.byref(out))[0] == INVALID
    assert out.value == 7.0
    for v, ones in ((a, np.ones(8, F32)), (b, np.ones(8, F64)), (short, np.ones(5, F32))):   # no refused call wrote anything
        assert v.to_numpy().tobytes() == ones.tobytes()
    short.add(short)
    a.add(short)                                                                             # x longer than y is legal
    assert a.to_numpy().tolist() == [3.0] * 5 + [1.0] * 3


def test_statuses_of_the_dev_entry_points(gpu):
    import torch
    L, INVALID = lib(), _lib.SMH_ERR_INVALID
    X, Y, A = Buf(np.ones(8, F32), 0, 5.0), Buf(np.ones(8, F32), 0, 5.0), Buf(np.array([2.0], F32), 0, 5.0)
    scratch = torch.zeros(L.smh_blas_dot_scratch_bytes(), dtype=torch.uint8, device="cuda")
    x, y, a, w = (C.c_void_p(p) for p in (X.ptr(), Y.ptr(), A.ptr(), scratch.data_ptr()))
    for fn in (L.smh_blas_axpy_dev, L.smh_blas_xpby_dev):
        assert status_of(fn, 7, x, a, y, 8, None) == (INVALID, "dtype must be SMH_F32 or SMH_F64")
        for args in ((None, a, y), (x, None, y), (x, a, None)):
            assert status_of(fn, _lib.SMH_F32, *args, 8, None) == (INVALID, "NULL device pointer")
        assert fn(_lib.SMH_F32, None, a, None, 0, None) == _lib.SMH_OK       # no entries: the vectors are not looked at
    assert status_of(L.smh_blas_dot_dev, -1, x, y, 8, a, w, None)[0] == INVALID
    for args in ((None, y, 8, a, w), (x, None, 8, a, w), (x, y, 8, None, w), (x, y, 8, a, None), (None, None, 0, None, w)):
        assert status_of(L.smh_blas_dot_dev, _lib.SMH_F32, *args, None) == (INVALID, "NULL device pointer")
    check(L.smh_blas_dot_dev(_lib.SMH_F32, None, None, 0, a, w, None))           # n == 0: +0, whatever the result held
    torch.cuda.synchronize()
    assert same(A.window(), np.zeros(1, F32))
    X.assert_untouched()
    Y.assert_untouched()


# ---- operands that overlap in part -------------------------------------------------------------------------------------------------
def vec_calls(a):
    L = lib()
    return [("smh_vec_add", lambda v, w: L.smh_vec_add(v._h, w._h), lambda x, y: bm.add(x, y)),
            ("smh_vec_sub", lambda v, w: L.smh_vec_sub(v._h, w._h), lambda x, y: bm.sub(x, y)),
            ("smh_vec_axpy", lambda v, w: L.smh_vec_axpy(v._h, a, w._h), lambda x, y: bm.axpy(x, a, y)),
            ("smh_vec_xpby", lambda v, w: L.smh_vec_xpby(v._h, a, w._h), lambda x, y: bm.xpby(x, a, y))]


@BOTH
def test_partly_overlapping_operands_are_refused(gpu, dtype):
    """smh_vec_add / sub / axpy / xpby and smh_blas_axpy_dev / xpby_dev: two windows of one buffer whose touched entries overlap in
    part -> SMH_ERR_INVALID and not a byte changed; the same pointer and disjoint windows, the neighbouring legal calls, go through.
    (The refused kernels are never launched: nothing here runs a race.)"""
    import torch
    a, n, s = 0.75, 16, bc.sentinel(dtype)
    data = bc.data(64, dtype, 49)
    A = Buf(np.array([a], dtype), 0, s)

    def dev(fn):
        return lambda v, w: fn(code(dtype), C.c_void_p(v.data_ptr()), C.c_void_p(A.ptr()), C.c_void_p(w.data_ptr()), min(len(v), len(w)), None)

    calls = vec_calls(a) + [("smh_blas_axpy_dev", dev(lib().smh_blas_axpy_dev), lambda x, y: bm.axpy(x, a, y)),
                            ("smh_blas_xpby_dev", dev(lib().smh_blas_xpby_dev), lambda x, y: bm.xpby(x, a, y))]
    for name, call, model in calls:
        B = Buf(data, 0, s)
        for xs, ys in ((0, 4), (4, 0), (0, 1), (1, 0), (0, n - 1), (n - 1, 0)):     # y ahead of x and behind it, by one entry and by n - 1
            status, text = status_of(call, B.vec(n, xs), B.vec(n, ys))
            assert status == _lib.SMH_ERR_INVALID and text == name + ": x and y overlap in part", (name, xs, ys)
            B.assert_untouched((name, xs, ys))
        # legal: adjacent windows, both ways round
        for xs, ys in ((0, n), (n, 0)):
            B = Buf(data, 0, s)
            check(call(B.vec(n, xs), B.vec(n, ys)))
            torch.cuda.synchronize()
            want = data.copy()
            want[xs:xs + n] = model(data[xs:xs + n], data[ys:ys + n])
            B.assert_window(want, len(data), (name, xs, ys))
        # legal: the same pointer through two handles
        B = Buf(data, 0, s)
        check(call(B.vec(n, 8), B.vec(n, 8)))
        torch.cuda.synchronize()
        want = data.copy()
        want[8:8 + n] = model(data[8:8 + n], data[8:8 + n].copy())
        B.assert_window(want, len(data), (name, "same pointer"))
    # only the entries that are touched count: y inside the part of a longer x that the operation leaves alone
    for name, call, model in vec_calls(a):
        B = Buf(data, 0, s)
        check(call(B.vec(32, 0), B.vec(8, 16)))
        want = data.copy()
        want[:32] = model(data[:32], data[16:24])
        B.assert_window(want, len(data), name)
        status, _ = status_of(call, B.vec(32, 0), B.vec(8, 4))      # ... and one that reaches into the touched entries
        assert status == _lib.SMH_ERR_INVALID
    A.assert_untouched()
