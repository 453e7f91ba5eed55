"""The model of the DenseVec kernels (tests/blas1_model.py), which tests/test_blas1_bits_gpu.py holds the device to bit for bit, checked
on the CPU -- and the cases of that test (tests/blas1_cases.py) checked for what they can see:

  1. dot against a plain Python walk of k_dot_stage1 / k_reduce_stage2 (grid -> thread -> vectors, tail, butterfly, waves), in both
     vector lengths and with operands of different length;
  2. every finite reduction case within tree_depth * eps * sum |x_i y_i| of cg_model.wide_dot (the exact sum rounded once): the
     standard bound of a sum of rounded products evaluated in any order, depth counted from the tree, nothing tuned;
  3. the scalar's single rounding and the entries an element-wise operation leaves alone;
  4. for sensitivity: every wrong variant of the model moves at least one bit in at least one case THAT THE DEVICE TEST RUNS, in the
     output the variant can affect.  The test prints, per variant, the cases that expose it.  Two variants cannot exist in f64 --
     "wide" (f32 terms accumulated in f64) and "scalar_double" (the API's double IS the f64 scalar) -- and the test asserts that
     they change nothing there instead."""
import math

import numpy as np
import pytest

import blas1_cases as bc
import blas1_model as bm
import cg_model as cm
from kernel_forms import same

F32, F64 = np.float32, np.float64
BOTH = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])


def differs(a, b):
    return not same(a, b)


# ---- 1. the literal walk ---------------------------------------------------------------------------------------------------------
def literal_workgroup(acc, T):
    waves = [list(acc[w * 64:(w + 1) * 64]) for w in range(4)]
    for v in waves:
        o = 32
        while o:
            v[:] = [T(v[l] + (v[l + o] if l + o < 64 else v[l])) for l in range(64)]  # (__shfl_down past the wave reads the lane itself)
            o //= 2
    r = T(0)
    for v in waves:
        r = T(r + v[0])
    return r


def literal_dot(x, y, aligned):
    T = x.dtype.type
    n = min(len(x), len(y))
    grid = max(1, min(1024, (n + 2047) // 2048))
    V = 16 // x.dtype.itemsize if aligned else 1
    partials = []
    with np.errstate(all="ignore"):
        for block in range(grid):
            acc = []
            for t in range(256):
                tid, a = block * 256 + t, T(0)
                i = tid
                while i < n // V:
                    for e in range(V):
                        a = T(a + T(x[i * V + e] * y[i * V + e]))
                    i += grid * 256
                i = (n // V) * V + tid
                while i < n:
                    a = T(a + T(x[i] * y[i]))
                    i += grid * 256
                acc.append(a)
            partials.append(literal_workgroup(acc, T))
        acc = []
        for t in range(256):
            a, i = T(0), t
            while i < grid:
                a = T(a + partials[i])
                i += 256
            acc.append(a)
        return literal_workgroup(acc, T)


@BOTH
@pytest.mark.parametrize("n", [0, 1, 3, 5, 257, 1027, 2049, 4101])
def test_dot_equals_the_literal_walk(n, dtype):
    x, y = bc.data(n, dtype, 1), bc.data(n + 3, dtype, 2)
    for aligned in (True, False):
        got = bm.dot(x, y, aligned)
        assert type(got) is dtype and same(got, literal_dot(x, y, aligned)), (n, aligned)
        assert same(bm.dot(y, x, aligned), got)  # the shorter operand decides, whichever side it is on
    assert same(bm.norm_squared(x), literal_dot(x, x, True)) and bm.norm(x) == math.sqrt(float(bm.norm_squared(x)))
    if n == 0:
        assert same(bm.dot(x, y), dtype(0)) and not np.signbit(bm.dot(x, y)) and bm.norm(x) == 0.0


@BOTH
def test_the_variants_helper_without_a_variant_is_the_tree(dtype):
    for n in (0, 1, 7, 2049, 70_001):
        x, y = bc.data(n, dtype, 3), bc.data(n, dtype, 4)
        for V in (1, cm.vec_len(dtype)):
            grid = cm.reduce_blocks(n)
            assert same(bm._wrong_sum(x, y, grid, V, False, False), cm.device_sum(x * y, grid, V)), (n, V)


# ---- 2. near the exact sum -------------------------------------------------------------------------------------------------------
@BOTH
def test_every_finite_reduction_case_is_near_the_exact_sum(dtype):
    eps, seen = float(np.finfo(dtype).eps), 0
    for case in bc.reduction_cases(dtype):
        x, y = case.arrays(dtype)
        n = min(len(x), len(y))
        x, y = x[:n], y[:n]
        if not (np.isfinite(x).all() and np.isfinite(y).all()) or case.name.startswith(("overflow", "subnormal")):
            continue
        got = bm.dot(x, y, case.aligned(dtype))
        V = cm.vec_len(dtype) if case.aligned(dtype) else 1
        scale = float(np.dot(np.abs(x).astype(np.longdouble), np.abs(y).astype(np.longdouble)))
        depth = cm.tree_depth(n, cm.reduce_blocks(n), V)
        assert abs(float(got) - float(cm.wide_dot(x, y))) <= depth * eps * scale, (case.name, got, depth)
        seen += 1
    assert seen >= len(bc.REDUCTION_SIZES) + len(bc.ALIGN_SIZES) * len(bc.offset_pairs(dtype))


# ---- 3. the scalar, and what an operation leaves alone ----------------------------------------------------------------------------
def test_the_scalar_is_rounded_once():
    a = 1.0 + 2.0 ** -24 + 2.0 ** -50        # above the midpoint of 1 and 1 + 2^-23: up.  (Rounded first to 1 + 2^-24 it would tie to 1.)
    assert bm.scalar(a, F32) == F32(1 + 2.0 ** -23) and bm.scalar(a, F64) == a
    assert bm.scalar(1e39, F32) == np.inf and bm.scalar(1e39, F64) == 1e39
    assert bm.scalar(1e-46, F32) == 0 and not np.signbit(bm.scalar(1e-46, F32)) and np.signbit(bm.scalar(-0.0, F32))
    assert np.isnan(bm.scalar(float("nan"), F32)) and float(bm.scalar(0.1, F32)) == float(F32(0.1)) != 0.1
    assert type(bm.scalar(F32(0.1), F32)) is F32 and bm.scalar(F32(0.1), F32) == F32(0.1)
    x = bc.data(9, F32, 5)
    assert same(bm.scale(x, a), x * F32(1 + 2.0 ** -23)) and same(bm.scale(x, 1e39), x * F32(np.inf))


@BOTH
def test_elementwise_model_touches_the_first_len_y_entries_only(dtype):
    x, y = bc.data(11, dtype, 6), bc.data(4, dtype, 7)
    a = bm.scalar(bc.EW_SCALAR, dtype)
    want = {"add": x[:4] + y, "sub": x[:4] - y, "axpy": x[:4] + y * a, "xpby": x[:4] * a + y, "rsub_into": y - x[:4]}
    for op, head in want.items():
        got = bm.ew(op, x, y, bc.EW_SCALAR)
        assert same(got[:4], head) and same(got[4:], x[4:]) and got is not x, op
    assert same(bm.scale(x, bc.EW_SCALAR), x * a)
    assert same(bm.axpy(x, a, y), bm.axpy(x, bc.EW_SCALAR, y))  # the _dev forms: the scalar is a T already


# ---- 4. what the device test's cases can see -----------------------------------------------------------------------------------------
def red_outputs(x, y, aligned, wrong):
    """what the device test reads back from a pair that the variants can change: the dot, both ways round"""
    nan = x.dtype.type(np.nan)
    return np.array([bm.dot(x, y, aligned, wrong, beyond=nan), bm.dot(y, x, aligned, wrong, beyond=nan)])


RIGHT = {}  # (type, case) -> the model's outputs, computed once for all variants


def exposing_reduction_cases(dtype, wrong, limit):
    """the cases whose outputs the variant changes; the sizes beyond `limit` are left to test_the_largest_sizes_tell_a_wrong_tree_too"""
    told, large = [], {"n%d" % n for n in bc.REDUCTION_SIZES if n > limit}
    for case in bc.reduction_cases(dtype):
        if case.name in large:
            continue
        x, y = case.arrays(dtype)
        if wrong == "fma" and not (np.isfinite(x).all() and np.isfinite(y).all() and case.group != "special"):
            continue  # (the emulated fused multiply-add is for finite data in the normal range)
        key = (np.dtype(dtype).name, case.name)
        if key not in RIGHT:
            RIGHT[key] = red_outputs(x, y, case.aligned(dtype), None)
        if differs(red_outputs(x, y, case.aligned(dtype), wrong), RIGHT[key]):
            told.append(case.name)
    return told


@BOTH
@pytest.mark.parametrize("wrong", bm.RED_WRONG)
def test_every_wrong_reduction_is_exposed_by_a_device_case(wrong, dtype):
    told = exposing_reduction_cases(dtype, wrong, 600_000)
    print("%s %s: %d cases: %s" % (np.dtype(dtype).name, wrong, len(told), " ".join(told)))
    if wrong == "wide" and dtype == F64:
        assert told == []  # (no wider type to accumulate in: the variant is the model)
        return
    assert told, wrong
    names = set(told)
    sizes = {n for n in bc.REDUCTION_SIZES if "n%d" % n in names}
    V = cm.vec_len(dtype)
    if wrong == "drop_tail":    # every aligned size with a tail, and no unaligned case (V = 1 has no tail)
        assert sizes == {n for n in bc.REDUCTION_SIZES if n % V and n <= 600_000}
    if wrong == "drop_last":
        assert sizes == {n for n in bc.REDUCTION_SIZES if 0 < n <= 600_000}
    if wrong == "aligned":      # only a pair with an operand off the boundary can tell
        unaligned = {c.name for c in bc.reduction_cases(dtype) if not c.aligned(dtype)}
        assert names <= unaligned and {"n%d-off1,0" % n for n in bc.ALIGN_SIZES} <= names
    if wrong == "no_truncate":
        assert {"trunc2049,1027", "trunc1027,2049"} <= names
    if wrong == "from_first":   # shows only in the sign of a zero, and only where EVERY thread of both stages holds a term
        assert told == ["minus-zeros-n%d" % bc.ALL_MINUS_ZERO_BIG]
    if wrong in ("sequential", "fma", "wide"):
        assert any(n <= 2048 for n in sizes) and any(n > 2048 for n in sizes)  # with one workgroup, and with several


@BOTH
def test_the_largest_sizes_tell_a_wrong_tree_too(dtype):
    """(the sizes the sensitivity test leaves out for its run time: the cap of 1024 workgroups and beyond)"""
    for n in (2_097_153, 4_198_403):
        x, y = bc.data(n, dtype, bc.SEED_X), bc.data(n, dtype, bc.SEED_Y)
        right = bm.dot(x, y)
        for wrong in ("drop_tail", "drop_last", "sequential"):
            assert differs(bm.dot(x, y, True, wrong), right), (n, wrong)
        assert differs(cm.device_sum(x * y, 2048, cm.vec_len(dtype)), right), n  # a grid that was not capped


@BOTH
def test_aligned_and_unaligned_models_differ_where_the_device_test_says_so(dtype):
    for n in bc.ALIGN_SIZES:
        x, y = bc.data(n, dtype, bc.SEED_X), bc.data(n, dtype, bc.SEED_Y)
        assert differs(bm.dot(x, y, True), bm.dot(x, y, False)), n


def ew_told(dtype, wrong):
    told, s = [], bc.sentinel(dtype)
    for case in bc.ew_cases(dtype):
        if case.n_x > 300_000:
            continue
        x, y = case.arrays(dtype)
        for op in ("add", "sub", "axpy", "xpby", "scale"):
            args = (x, None) if op == "scale" else (x, y)
            if differs(bm.ew(op, *args, a=bc.EW_SCALAR, wrong=wrong, beyond=s), bm.ew(op, *args, a=bc.EW_SCALAR)):
                told.append("%s/%s" % (case.name, op))
    x, y = bc.data(bc.SCALAR_SIZE, dtype, 43), bc.data(bc.SCALAR_SIZE, dtype, 44)
    for a in bc.SCALARS:
        for op in ("axpy", "xpby", "scale"):
            args = (x, None) if op == "scale" else (x, y)
            if wrong != "fma" and differs(bm.ew(op, *args, a=a, wrong=wrong, beyond=s), bm.ew(op, *args, a=a)):
                told.append("scalar%r/%s" % (a, op))
    return told


@BOTH
@pytest.mark.parametrize("wrong", bm.EW_WRONG)
def test_every_wrong_elementwise_is_exposed_by_a_device_case(wrong, dtype):
    told = ew_told(dtype, wrong)
    print("%s %s: %d cases: %s" % (np.dtype(dtype).name, wrong, len(told), " ".join(told[:40])))
    if wrong == "scalar_double" and dtype == F64:
        assert told == []
        return
    assert told, wrong
    ops = {t.split("/")[1] for t in told}
    if wrong == "fma":
        assert ops == {"axpy", "xpby"}
    if wrong == "scalar_double":
        assert ops == {"axpy", "xpby", "scale"} and any(t.startswith("scalar%r/" % bc.SCALARS[2]) for t in told)
    if wrong == "xpby_swapped":
        assert ops == {"xpby"}
    if wrong == "past_rhs":     # only a right-hand side that ends before x does can tell
        assert ops == {"add", "sub", "axpy", "xpby"} and all(t.startswith("short") for t in told)
        assert any(t.startswith("short1027-into4101/") for t in told) and any(t.startswith("short1027-into4101-off1,0/") for t in told)


@BOTH
def test_special_pairs_reach_the_subnormals_the_zeros_and_the_overflow(dtype):
    """the element-wise special-value sweep of the device test meets what it says it meets: a flushed subnormal, a lost sign of zero
    or a saturated overflow would each change a bit of the expected result"""
    x, y = bc.special_pairs(dtype)
    tiny = np.finfo(dtype).tiny
    assert len(x) % cm.vec_len(F32) and len(x) % cm.vec_len(F64)

    def subnormal(v):
        return (v != 0) & (np.abs(v) < tiny)

    normal_in = ~subnormal(x) & ~subnormal(y) & np.isfinite(x) & np.isfinite(y)
    s = bm.add(x, y)
    assert (subnormal(s) & subnormal(x)).any() and (np.isinf(s) & normal_in).any() and np.isnan(s).any()
    assert np.signbit(s[s == 0]).any() and (~np.signbit(s[s == 0])).any()
    p = bm.scale(x, 0.5)
    assert (subnormal(p) & ~subnormal(x)).any() and ((p == 0) & (x != 0)).any()           # underflow to a subnormal, and to zero
    assert (np.isinf(bm.scale(x, 2.0)) & np.isfinite(x)).any()
    q = bm.axpy(x, float(tiny), y)
    assert (subnormal(q) & normal_in).any()
    flushed = np.where(subnormal(q), dtype(0), q)
    assert differs(flushed, q)
    for a in bc.special_scalars(dtype):
        for op in ("axpy", "xpby"):
            assert bm.ew(op, x, y, a).dtype == np.dtype(dtype)
