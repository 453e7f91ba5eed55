"""numpy restatement of the k-column conjugate gradient (sparsemat_amd/csrc/cg_many.hip) and of the column tree that it shares
with MultiVec.dot / norm_squared (mvec_blas.hip) -- test infrastructure, not product code.  Built from cg_model's primitives.

Column c of a solve is ConjugateGradient::solve (linearsolver.rs:27-61) on (A, b_c, x_c), nothing else: the model runs the
columns one after the other, so it CANNOT let one column reach another.  Every reduction of a column is ``column_sum``:

  B = cg_update_grid(n) workgroups of 256 threads; thread g = 256 w + t starts from T(0) and adds the rounded terms of rows
  g, g + 256 B, ... in that order; a wavefront folds by __shfl_down (32, ..., 1); thread 0 adds the four wave sums from T(0);
  one workgroup folds the B partials the same way.  The order depends on n alone.

Unlike the single solver's model there is no one-value re-fold (``Reducer.one``): p.Ap's partials are folded once, by the
update kernel.  Ap comes from oracle.spmv per column (K1m is bit for bit that).
"""
import math

import numpy as np

import oracle
from cg_model import cg_update_grid, device_sum, sequential_sum


def column_sum(terms, mode="device"):
    """The sum of one column's rounded terms as the device builds it ("device") or as a left-to-right fold ("sequential")."""
    terms = np.ascontiguousarray(terms)
    if mode == "sequential":
        return sequential_sum(terms)
    assert mode == "device"
    return device_sum(terms, cg_update_grid(len(terms)), 1)


class ColumnResult:
    def __init__(self, x, r, p, iterations, rr):
        self.x, self.r, self.p, self.iterations, self.rr = x, r, p, iterations, rr
        self.r_norm_squared = float(rr)


def cg_column(off, col, val, b, x0, tol, iter_max, mode):
    val = np.ascontiguousarray(val)
    T = val.dtype.type
    with np.errstate(all="ignore"):  # (0 / 0 is the reference's behaviour for b = 0, not an accident)
        x = np.array(x0, val.dtype, copy=True)
        b = np.ascontiguousarray(b, val.dtype)
        r = b - oracle.spmv(off, col, val, x)          # :38
        p = r.copy()                                   # :39
        rr = column_sum(r * r, mode)                   # :40
        iters = 0
        while iters < iter_max:
            iters += 1
            ap = oracle.spmv(off, col, val, p)         # :43
            pap = column_sum(p * ap, mode)
            alpha = T(rr / pap)                        # :45
            r = r - ap * alpha                         # :49
            rr_new = column_sum(r * r, mode)           # :51
            x = x + p * alpha                          # :47 (every entered body)
            rr_old, rr = rr, rr_new
            if math.sqrt(float(rr)) < tol:             # :52-54, before beta
                break
            beta = T(rr / rr_old)                      # :56
            p = p * beta + r                           # :58-59
    return ColumnResult(x, r, p, iters, rr)


class Result:
    """x: (k, n); iterations: int64 (k,); r_norm_squared: f64 (k,)."""

    def __init__(self, cols, n, dtype):
        self.columns = cols
        self.x = np.stack([c.x for c in cols]) if cols else np.zeros((0, n), dtype)
        self.iterations = np.array([c.iterations for c in cols], np.int64)
        self.r_norm_squared = np.array([c.r_norm_squared for c in cols], np.float64)


def cg_many(off, col, val, B, X0, tol, iter_max, mode="device"):
    """B, X0: (k, n).  The k independent solves of smh_cg_solve_many."""
    val = np.ascontiguousarray(val)
    B = np.asarray(B, val.dtype)
    X0 = np.asarray(X0, val.dtype)
    assert B.ndim == 2 and B.shape == X0.shape
    return Result([cg_column(off, col, val, B[c], X0[c], tol, iter_max, mode) for c in range(B.shape[0])], B.shape[1], val.dtype)
