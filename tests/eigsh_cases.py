"""The cases tests/test_eigsh_gpu.py compares bit for bit with eigsh_model's "device" mode -- shared with tests/test_eigsh_model.py,
which shows (without a GPU) that each of them moves a bit under every wrong variant of the arithmetic that can touch it -- and the
convergence cases of the CPU file.

V = 16 bytes / sizeof(T): 4 in f32, 2 in f64; kBlock = 256 threads; the dots' tile is 8 columns (gmres_model.TILE), the rotation's
output tile 8 columns (eigsh_model.ROT_TILE); a restart keeps l = k + (m - k) // 2 columns."""
import numpy as np

import eigsh_model as em

F32, F64 = np.float32, np.float64
LA, SA = em.LARGEST, em.SMALLEST


class Case:
    """matrix(dtype) -> (off, col, val); start(dtype); k, ncv, which, tol(dtype), restart_max.  exact: every number of the solve is
    exact in any order, or nothing is returned, so no wrong variant can show"""

    def __init__(self, name, n, build, k, ncv, which=LA, tol=(0.0, 0.0), restart_max=2, start=None, exact=False):
        self.name, self.n, self.build, self.k, self.ncv, self.which, self.tols = name, n, build, k, ncv, which, tol
        self.restart_max, self.start_of, self.exact = restart_max, start, exact

    def matrix(self, dtype):
        return self.build(self.n, dtype)

    def start(self, dtype):
        if self.start_of is not None:
            return np.asarray(self.start_of(self.n), dtype)
        return em.start_vector(self.n, dtype, seed=self.n % 89)

    def tol(self, dtype):
        return self.tols[0] if dtype == F32 else self.tols[1]

    def m(self):
        return em.clip_ncv(self.n, self.k, self.ncv)

    def l(self):
        return self.k + (self.m() - self.k) // 2


def tri(n, dtype):
    return em.tridiag_sym(n, dtype, seed=n % 97)


def run_model(case, dtype, **kw):
    off, col, val = case.matrix(dtype)
    return em.eigsh(off, col, val, case.start(dtype), case.k, case.ncv, case.which, case.tol(dtype), case.restart_max, **kw)


# ---- the bit cases ---------------------------------------------------------------------------------------------------------
# tol = 0: a pair converges only on an estimate that is exactly zero, so a case runs exactly restart_max restarts.
# sizes: 1, 2, 3 (m = n: the first cycle is the whole space), 5; eight consecutive n around 257 (one and two workgroups, every
# n mod V, fewer vectors than lanes); 2049 / 2051 (nine workgroups)
SIZES = [Case("n=%d" % n, n, tri, 1 if n < 3 else 2, 6, LA if n % 2 else SA) for n in (1, 2, 3, 5, 253, 254, 255, 256, 257, 258, 259, 260, 2049, 2051)]
# basis widths on n = 130: (k, m) with l and m around the dots' tile of 8 columns and the rotation's output tile of 8; (1, 3) has
# l = 2 = m - 1, a one-body cycle; k = 3, 4, 5: an smh_mvec with and without padding columns; m = 128 once, one restart
WIDTHS = [Case("k=%d m=%d" % (k, m), 130, tri, k, m, which) for k, m, which in
          ((1, 3, LA), (2, 7, SA), (3, 8, LA), (4, 9, SA), (5, 12, LA), (7, 9, SA), (6, 13, LA), (3, 17, SA), (9, 25, LA))]
# (k = 30: after 128 of 130 dimensions the first estimates underflow to exactly zero -- converged even at tol = 0 -- the 30th does not)
WIDEST = Case("k=30 m=128", 130, tri, 30, 128, LA, restart_max=1)
# stops: converged inside the restart budget (the tolerances of the convergence cases), restart_max 0 and 1 (n_conv < k)
STOPS = [
    Case("converges LA", 100, tri, 4, 20, LA, tol=(1e-4, 1e-10), restart_max=200),
    Case("converges SA", 100, tri, 4, 20, SA, tol=(1e-4, 1e-10), restart_max=200),
    Case("restart_max 0", 100, tri, 4, 20, LA, tol=(1e-4, 1e-10), restart_max=0),
    Case("restart_max 1", 100, tri, 4, 20, SA, tol=(1e-4, 1e-10), restart_max=1),
    Case("default ncv", 100, tri, 3, 0, LA, tol=(1e-4, 1e-10), restart_max=3),
]


DIAG = [-2.0, 7.0, 0.0, 9.0, 2.0, 5.0, 6.0, 8.0]


def diag8(n, dtype):
    """diag(DIAG), every diagonal entry stored (the zero too)"""
    return np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.array(DIAG[:n], dtype)


def three_entries(n):
    """(3, 2, 3) on the entries whose eigenvalues are -2, 0, 2: v_0 and A v_0 are symmetric / antisymmetric about the middle entry, so
    the dots that vanish in exact arithmetic vanish in floating point too, in every order of the sums, and the third body's w is
    exactly zero (found by search among small integers; a start whose normalisation is exact cannot have three entries)"""
    v = np.zeros(n)
    v[[0, 2, 4]] = (3.0, 2.0, 3.0)
    return v


def two_i(n, dtype):
    return em.crs_from_dense(2 * np.eye(n), dtype)


def e1(n):
    v = np.zeros(n)
    v[0] = 1
    return v


def with_nan(n, dtype):
    off, col, val = tri(n, dtype)
    val[len(val) // 2] = np.nan
    return off, col, val


EXACT = [
    # the Krylov space of three eigenvectors is exhausted after three bodies: breakdown 1, the three eigenvalues 2, 0, -2
    Case("diag, start on three entries, k=2", 8, diag8, 2, 6, LA, tol=(1e-4, 1e-10), start=three_entries),
    # ... with k = 4 > 3 columns: the values past the third are NaN, the vectors past it signed zeros (the zero coefficients)
    Case("diag, start on three entries, k=4", 8, diag8, 4, 7, SA, tol=(1e-4, 1e-10), start=three_entries),
    Case("A = 2 I", 5, two_i, 1, 4, LA, tol=(1e-6, 1e-6), start=e1, exact=True),
    Case("zero start", 5, two_i, 1, 4, LA, start=lambda n: np.zeros(n), exact=True),
    Case("infinite start", 5, two_i, 1, 4, LA, start=lambda n: np.full(n, np.inf), exact=True),
    Case("NaN in the matrix", 259, with_nan, 2, 6, SA, exact=True),
]
BIT_CASES = SIZES + WIDTHS + [WIDEST] + STOPS + EXACT

# ---- the convergence cases of the CPU file: (name, build, n) x which x (k, m), tol 1e-4 in f32 and 1e-10 in f64 --------------
CONVERGENCE = [("tridiag 100", lambda dtype: em.tridiag_sym(100, dtype, seed=0), 100),
               ("tridiag 263", lambda dtype: em.tridiag_sym(263, dtype, seed=0), 263),
               ("grid 24 x 20", lambda dtype: em.grid_operator(24, 20, dtype, seed=0), 480)]
KM = [(1, 8), (4, 20), (8, 24)]


def conv_tol(dtype):
    return 1e-4 if dtype == F32 else 1e-10
