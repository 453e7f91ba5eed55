"""The cases tests/test_refine_gpu.py compares bit for bit with tests/refine_model.py -- shared with tests/test_refine_model.py,
which shows (without a GPU) that each of them moves a bit, or a count, under every wrong variant of the arithmetic that can touch it.

A case is a system in f64 (off, col, val, b, x0), the choice of inner solver and preconditioner, and the knobs.  ``inner_of`` builds the
model's inner solve from the f32 values, the factors' values and a source of products -- the oracle's on the CPU, the device's own,
checked, on the GPU."""
import numpy as np

import bicgstab_model as bm
import cg_model
import fsai_model as fm
import fsai_ns_model as nm
import ilu_model
import pgmres_model as pm
import refine_model as rm

F32, F64 = np.float32, np.float64
ALL_WRONG = ("residual_f32", "sequential", "e_up", "warm_start", "no_x_prev")


def rhs(n, seed):
    rng = np.random.default_rng(4000 + seed)
    return rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)


def tridiag(n):
    """cg_model.tridiag in f64 (SPD, a random diagonal: the f32 copy rounds), b random, x0 = 0"""
    off, col, val = cg_model.tridiag(n, F64, seed=n % 89)
    b, _ = rhs(n, n % 89)
    return off, col, val, b, np.zeros(n)


def tridiag_x0(n):
    off, col, val, b, _ = tridiag(n)
    return off, col, val, b, rhs(n, n % 89)[1]


def convdiff(n):
    """convdiff2d(24, 1.0), rows sorted, b random, x0 = 0"""
    off, col, val = pm.sort_rows(*bm.convdiff2d(24, 1.0, F64))
    return off, col, val, rhs(576, 24)[0], np.zeros(576)


def convdiff_sym(n):
    """S (A + A^T) / 2 S of the same operator with S = diag(1 + u / 4): SPD, values that round in f32"""
    off, col, val = pm.sort_rows(*bm.convdiff2d(24, 0.0, F64))  # (c = 0: the pattern with symmetric values)
    rows = np.repeat(np.arange(576), np.diff(off.astype(np.int64)))
    sym = np.where(col == rows, 5.0, np.where(np.abs(col.astype(np.int64) - rows) == 1, -1.5, -1.0))
    s = 1.0 + np.random.default_rng(5).uniform(0, 0.25, 576)
    return off, col, sym * s[rows] * s[col], rhs(576, 25)[0], np.zeros(576)


def zero_b(n):
    off, col, val, b, x0 = tridiag(n)
    return off, col, val, np.zeros(n), x0


def nan_b(n):
    off, col, val, b, _ = tridiag_x0(n)
    b = b.copy()
    b[n // 2] = np.nan
    return off, col, val, b, rhs(n, 3)[1]


class Case:
    """wrong: the wrong variants of refine_model.WRONG that move a bit or a count of this case"""

    def __init__(self, name, build, n, inner="cg", precond=None, tol=1e-9, outer_max=0, inner_tol=0.0, inner_iter_max=0, restart=0, wrong=ALL_WRONG,
                 code=0):
        self.name, self.build, self.n, self.inner, self.precond, self.tol = name, build, n, inner, precond, tol
        self.outer_max, self.inner_tol, self.inner_iter_max, self.restart, self.wrong, self.code = outer_max, inner_tol, inner_iter_max, restart, wrong, code

    def system(self):
        return self.build(self.n)

    def factors(self, off, col, val32):
        """the model's f32 factors of the f32 matrix: None, (off, col, fval) for ILU, a pair of such for FSAI"""
        if self.precond == "ilu":
            return off, col, ilu_model.ilu0(off, col, val32)[0]
        if self.precond == "fsai" and self.inner == "cg":
            goff, gcol, gval, bad = fm.fsai(off, col, val32)
            assert bad is None
            return (goff, gcol, gval), fm.transpose(goff, gcol, gval)
        if self.precond == "fsai":
            gl, gu, bad = nm.fsai_ns(off, col, val32)
            assert bad is None
            return gl, gu
        return None

    def inner_of(self, off, col, val32, factors, product, fused=False):
        """The model's inner solve.  product(off, col, val, kind) -> (v -> A v): kind "matrix" for the f32 matrix (by variant_lo), "body"
        for a factor applied inside a body, "end" for GMRES's cycle end."""
        tol = self.inner_tol or rm.DEFAULT_INNER_TOL
        iter_max = self.inner_iter_max or rm.DEFAULT_INNER_ITER_MAX
        mvp = product(off, col, val32, "matrix")
        apply = end = None
        if self.precond == "jacobi":
            apply = pm.jacobi(off, col, val32)
        elif self.precond == "sgs":
            apply = pm.sgs(off, col, val32)
        elif self.precond == "ilu":
            apply = pm.ilu(*factors)
        elif self.precond == "fsai":
            first, second = product(*factors[0], "body"), product(*factors[1], "body")
            apply = lambda v: second(first(v))
            first_end, second_end = product(*factors[0], "end"), product(*factors[1], "end")
            end = lambda v: second_end(first_end(v))
        if self.inner == "cg":
            if self.precond is None:
                return rm.inner_cg(off, col, val32, tol, iter_max, mvp, fused)
            return rm.inner_pcg(off, col, val32, apply, tol, iter_max, mvp, fused)
        if self.inner == "bicgstab":
            return rm.inner_bicgstab(off, col, val32, apply, tol, iter_max, mvp)
        return rm.inner_gmres(off, col, val32, self.restart or 30, apply, end if self.precond == "fsai" else None, tol, iter_max, mvp)


# Which wrong variants a case can tell from the right arithmetic (tests/test_refine_model.py holds every entry to it).  "sequential"
# shows only while the residual is large: b - A x of a nearly solved system is a vector of small multiples of one power of two, whose
# squares add up exactly in any order -- the cases that stop at outer 0 or 1 show it.  "e_up" needs an r.r with an odd exponent at some
# outer step; "warm_start" a second inner solve; "no_x_prev" a stall.  n <= 3: the inner solve is exact to f32 at once.
R, S, E, W, N = ALL_WRONG
_TRIDIAG_WRONG = {0: (), 1: (R,), 3: (R, W), 259: (R, W), 260: (R, W)}

# CG on cg_model.tridiag at every path size of the sweeps: no rows, one workgroup around every n mod 16 bytes, nine workgroups, a second
# trip of the grid (512 workgroups x 256 threads x 2 elements = 262 144)
SIZES = [Case("tridiag%d" % n, tridiag, n, wrong=_TRIDIAG_WRONG.get(n, (R, E, W))) for n in [0, 1, 3] + list(range(257, 265)) + [2051]]
# (the large one: two outer steps of six bodies each, so that the GPU test's checked products stay few)
SIZES.append(Case("tridiag262447", tridiag, 262447, outer_max=2, inner_iter_max=6, code=1, wrong=(R, S, W)))

# one case per inner solver and preconditioner, on convdiff2d(24, 1.0) or its symmetric part
KINDS = [
    Case("cg+sgs", convdiff_sym, 576, "cg", "sgs", wrong=(R, E, W)),
    Case("cg+ilu", convdiff_sym, 576, "cg", "ilu", wrong=(R, W)),
    Case("cg+fsai", convdiff_sym, 576, "cg", "fsai", wrong=(R, E, W)),
    Case("bicgstab+jacobi", convdiff, 576, "bicgstab", "jacobi", wrong=(R, E, W)),
    Case("bicgstab+fsai", convdiff, 576, "bicgstab", "fsai", wrong=(R, W)),
    Case("gmres5", convdiff, 576, "gmres", None, restart=5, wrong=(R, E, W)),
    Case("gmres30+ilu", convdiff, 576, "gmres", "ilu", restart=30, wrong=(R, E, W)),
]

# the stops
STOPS = [
    Case("tol_met", tridiag, 260, tol=1e3, wrong=(R, S)),                           # outer 0, no inner call: rr alone can move
    Case("outer_max1", tridiag, 260, outer_max=1, code=1, wrong=(R, S)),
    Case("stall", tridiag, 260, tol=0.0, code=2, wrong=(R, W, N)),                  # until a step no longer lowers r.r
    Case("zero_b", zero_b, 260, wrong=()),                                          # rr == 0 at once
    Case("nan_b", nan_b, 260, inner_iter_max=5, code=2, wrong=(N,)),                # x = x0 comes back
    Case("x0", tridiag_x0, 261, wrong=(R, E, W)),
    Case("loose_inner", tridiag, 259, inner_tol=1e-2, wrong=(R, E, W)),
]

CASES = SIZES + KINDS + STOPS
BY_NAME = {c.name: c for c in CASES}


def oracle_products(off, col, val, kind):
    import oracle
    return lambda v: oracle.spmv(off, col, val, np.ascontiguousarray(v, val.dtype))


def model(case, wrong=None, system=None):
    """The model on the CPU: the oracle's products, the models' factors."""
    off, col, val, b, x0 = system or case.system()
    val32 = rm.cast(val, F32)
    inner = case.inner_of(off, col, val32, case.factors(off, col, val32), oracle_products)
    return rm.refine(oracle_products(off, col, val, "matrix"), inner, b, x0, case.tol, case.outer_max, wrong=wrong)
