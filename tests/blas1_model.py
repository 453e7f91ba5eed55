"""numpy restatement of the DenseVec kernels (K3 / K4 of sparsemat_amd/csrc/blas1.hip) as the public entry points reach them:
smh_vec_add / sub / scale / axpy / xpby / dot / norm_squared / norm and smh_blas_dot_dev / axpy_dev / xpby_dev (the same file) -- test
infrastructure, not product code.  The reduction tree is tests/cg_model.py's (device_sum, reduce_blocks, vec_len), which the solvers'
tests pin; what is written here is what this layer adds: which entries an operation touches, how the scalar arrives, which vector
length a pair of buffers selects.  All arithmetic is in T with one rounding per multiply and one per add (the library is built with
-ffp-contract=off, the kernels call the *_rn intrinsics).

  element-wise   k_ew over the first len(y) entries of x (zip truncation: densevec.rs:52-54), entry by entry, no entry depends on
                 another, so the grid and the vector path cannot change a bit -- what they can do wrong is WHERE they write; the
                 rest of x comes back untouched.  The API's scalar is a double and is rounded ONCE to T, `(T)a` at the launch; the
                 _dev forms read a T from device memory.
                   add   x + y            sub        x - y            scale  round(x * a), over ALL of x
                   axpy  x + round(y * a) xpby  round(x * a) + y      rsub_into  y - x
  dot            terms x_i * y_i rounded to T over n = min(len(x), len(y)) (vector.rs:52), summed by launch_dot's tree:
                 reduce_blocks(n) workgroups; a thread strides over vectors of V = 16 bytes / sizeof(T) elements and then takes one
                 tail element when BOTH buffers are 16-byte aligned (k_dot_stage1<T, true>), over single elements (V = 1) when one
                 of them is not; every accumulator starts at +0.  n == 0: the tree of no terms, +0.
  norm_squared   dot(x, x) (the kernel reads x once when both pointers are equal: the same terms)
  norm           sqrt in double of the norm_squared widened to double (vector.rs:61-63)

`wrong=`: a named mistake instead, ONLY for showing that a test case tells it apart (tests/test_blas1_model.py)."""
import math

import numpy as np

import cg_model as cm
import inner_prod_model as ipm

F32, F64 = np.float32, np.float64

EW_OPS = ("add", "sub", "scale", "axpy", "xpby", "rsub_into")
# fma: one rounding for multiply and add (axpy, xpby); scalar_double: the product formed with the API's double scalar and rounded
# to T afterwards, the scalar itself never rounded (f32 only: in f64 the double IS the T); xpby_swapped: x + round(b * y), axpy's
# shape; past_rhs: the sweep covers len(x) entries, reading `beyond` where y has ended
EW_WRONG = ("fma", "scalar_double", "xpby_swapped", "past_rhs")
# aligned: V as if both buffers were aligned; drop_tail: the n % V tail elements missing; drop_last: the vector one entry short;
# fma: acc = fma(x, y, acc); wide: the f32 terms accumulated in f64, rounded at the end (f32 only); sequential: the reference's left
# fold; from_first: a fold starts at its first term, not at +0 (a thread's run and thread 0's sum of the waves); no_truncate: len(x)
# terms, y continued by `beyond`
RED_WRONG = ("aligned", "drop_tail", "drop_last", "fma", "wide", "sequential", "from_first", "no_truncate")


def scalar(a, dtype):
    """the API's double as the kernel receives it: rounded once to T (1e39 is +Inf in f32, 1e-46 is +0); a T stays what it is"""
    with np.errstate(all="ignore"):
        return np.dtype(dtype).type(a)


# ---- element-wise ----------------------------------------------------------------------------------------------------------------
def _apply(op, x, y, a, a_double, wrong):
    T = x.dtype.type
    if op == "add":
        return x + y
    if op == "sub":
        return x - y
    if op == "rsub_into":
        return y - x
    if op == "scale":
        if wrong == "scalar_double":
            return (x.astype(F64) * a_double).astype(x.dtype)
        return x * a
    if op == "xpby" and wrong == "xpby_swapped":
        return x + y * a
    m, z = (y, x) if op == "axpy" else (x, y)        # round(m * a) + z
    if wrong == "fma":
        return ipm.fma(m, np.full(len(m), a, x.dtype), z)
    if wrong == "scalar_double":
        return (m.astype(F64) * a_double).astype(x.dtype) + z
    assert T is type(a)
    return m * a + z


def ew(op, x, y=None, a=0.0, wrong=None, beyond=None):
    """x after `op`, a new array of len(x): the first len(y) entries computed (scale: all of them), the others as they were.
    a: the API's double, or a T for the _dev forms.  beyond: what a sweep that runs past the end of y would read (past_rhs)."""
    assert op in EW_OPS and wrong in (None,) + EW_WRONG
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.dtype(F32), np.dtype(F64)) and (y is None) == (op == "scale")
    y = x if y is None else np.ascontiguousarray(y)
    assert y.dtype == x.dtype and len(y) <= len(x)
    n = len(y)
    if wrong == "past_rhs" and op != "scale":
        y = np.concatenate([y, np.full(len(x) - n, beyond, x.dtype)])
        n = len(x)
    out = x.copy()
    with np.errstate(all="ignore"):
        out[:n] = _apply(op, x[:n], y[:n], scalar(a, x.dtype), float(a), wrong)
    return out


def add(x, y, **kw):
    return ew("add", x, y, **kw)


def sub(x, y, **kw):
    return ew("sub", x, y, **kw)


def rsub_into(x, y, **kw):
    return ew("rsub_into", x, y, **kw)


def scale(x, a, **kw):
    return ew("scale", x, None, a, **kw)


def axpy(x, a, y, **kw):
    """x += round(a * y)"""
    return ew("axpy", x, y, a, **kw)


def xpby(x, b, y, **kw):
    """x = round(b * x) + y"""
    return ew("xpby", x, y, b, **kw)


# ---- reductions ------------------------------------------------------------------------------------------------------------------
def _thread_runs(x, y, grid, V, fused, from_first):
    """the per-thread sums of a grid-stride sweep over vectors of V products and one tail element (cm.thread_sums), with a mistake in
    them: acc = fma(x, y, acc) (fused), or a run that starts at its first term instead of +0 (from_first)"""
    n, nthreads = len(x), grid * cm.K_BLOCK
    nv = n // V
    acc = np.zeros(nthreads, x.dtype)
    started = np.zeros(nthreads, bool)

    def step(acc, started, a, b, live):
        new = ipm.fma(a, b, acc) if fused else acc + a * b
        if from_first:
            new = np.where(started, new, a * b)
        return np.where(live, new, acc), started | live

    trips = (nv + nthreads - 1) // nthreads
    if trips:
        xs, ys = np.zeros((2, trips * nthreads * V), x.dtype)
        xs[:nv * V], ys[:nv * V] = x[:nv * V], y[:nv * V]
        live = (np.arange(trips * nthreads * V) < nv * V).reshape(trips, nthreads, V)
        xs, ys = xs.reshape(trips, nthreads, V), ys.reshape(trips, nthreads, V)
        for k in range(trips):
            for e in range(V):
                acc, started = step(acc, started, xs[k, :, e], ys[k, :, e], live[k, :, e])
    tail = n - nv * V
    if tail:
        acc[:tail], started[:tail] = step(acc[:tail], started[:tail], x[nv * V:], y[nv * V:], np.ones(tail, bool))
    return acc


def _wrong_sum(x, y, grid, V, fused, from_first):
    """launch_dot's two stages with one of the two mistakes in every fold it has (the fold of the partials is a sweep over
    partial * 1).  With neither it is cm.device_sum of the rounded products (tests/test_blas1_model.py holds it to that)."""
    parts = cm.block_sums(_thread_runs(x, y, grid, V, fused, from_first), from_first)
    return cm.block_sums(_thread_runs(parts, np.ones(len(parts), x.dtype), 1, 1, False, from_first), from_first)[0]


def dot(x, y, aligned=True, wrong=None, beyond=None):
    """smh_vec_dot / smh_blas_dot_dev as a T.  aligned: BOTH device pointers are 16-byte aligned."""
    assert wrong in (None,) + RED_WRONG
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.dtype == y.dtype and x.dtype in (np.dtype(F32), np.dtype(F64))
    T = x.dtype.type
    n = min(len(x), len(y))
    if wrong == "no_truncate":
        n = len(x)
        y = np.concatenate([y, np.full(max(0, n - len(y)), beyond, x.dtype)])
    x, y = x[:n], y[:n]
    V = cm.vec_len(x.dtype) if aligned or wrong == "aligned" else 1
    grid = cm.reduce_blocks(n)
    with np.errstate(all="ignore"):
        if wrong == "drop_tail":
            x, y = x[:n - n % V], y[:n - n % V]
        if wrong == "drop_last":
            x, y = x[:max(n - 1, 0)], y[:max(n - 1, 0)]
            grid = cm.reduce_blocks(len(x))
        if wrong in ("fma", "from_first"):
            return T(_wrong_sum(x, y, grid, V, wrong == "fma", wrong == "from_first"))
        terms = x * y
        if wrong == "sequential":
            return T(cm.sequential_sum(terms))
        if wrong == "wide":
            return T(cm.device_sum(terms.astype(F64), grid, V))
        return T(cm.device_sum(terms, grid, V))


def norm_squared(x, aligned=True, wrong=None):
    return dot(x, x, aligned, wrong)


def norm(x, aligned=True):
    """a double: f64::sqrt(self.norm_squared().into())"""
    return math.sqrt(float(norm_squared(x, aligned)))
