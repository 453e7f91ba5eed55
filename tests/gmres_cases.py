"""The cases tests/test_gmres_gpu.py compares bit for bit with gmres_model's "device" mode -- shared with tests/test_gmres_model.py,
which shows (without a GPU) that each of them moves a bit under every wrong variant of the arithmetic it can tell apart.

V = 16 bytes / sizeof(T): 4 in f32, 2 in f64; kBlock = 256 threads; gmres_model.TILE = 8 columns per load of w in the dots."""
import numpy as np

import bicgstab_model as bm
import gmres_model as gm

F32, F64 = np.float32, np.float64


def vec_len(dtype):
    return 16 // np.dtype(dtype).itemsize


def rhs(n, dtype, seed):
    rng = np.random.default_rng(2000 + seed)
    return rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)


class Case:
    """system(dtype) -> (off, col, val, b, x0); tol(dtype); restart; iter_max; exact: every number of the solve is exact in any
    order (small integers), so no wrong variant can show"""

    def __init__(self, name, n, build, restart, iter_max, tol=(0.0, 0.0), exact=False):
        self.name, self.n, self.build, self.restart, self.iter_max, self.tols, self.exact = name, n, build, restart, iter_max, tol, exact

    def system(self, dtype):
        return self.build(self.n, dtype)

    def tol(self, dtype):
        return self.tols[0] if dtype == F32 else self.tols[1]


def ns(n, dtype):
    """tridiag_ns(n, .5): diagonally dominant, not symmetric; b and a NON-ZERO x0 random"""
    off, col, val = bm.tridiag_ns(n, 0.5, dtype, seed=n % 97)
    b, x0 = rhs(n, dtype, n % 97)
    return off, col, val, b, x0


def skew(n, dtype):
    """tridiag(-1, .125, +1), b random, x0 random: hundreds of bodies to converge, so a cycle never ends early"""
    off, col, val = gm.tridiag_skew(n, 0.125, dtype)
    b, x0 = rhs(n, dtype, 7)
    return off, col, val, b, x0


def convdiff5(n, dtype):
    off, col, val, b, _ = bm.convdiff_system(5, 0.5, dtype)
    return off, col, val, b, np.zeros(n, dtype)


def two_i(n, dtype):
    off, col, val = bm.dense_to_crs(2 * np.eye(n), dtype)
    b = np.zeros(n, dtype)
    b[0] = 1
    return off, col, val, b, np.zeros(n, dtype)


def skew2(n, dtype):
    off, col, val = bm.dense_to_crs([[0, 1], [-1, 0]], dtype)
    return off, col, val, np.array([1, 0], dtype), np.zeros(2, dtype)


def solved(n, dtype):
    """b = A x0 exactly: beta == 0 at the set-up"""
    off, col, val = bm.dense_to_crs([[2, 1], [0, 3]], dtype)
    return off, col, val, np.array([4, 3], dtype), np.array([1.5, 1.0], dtype)


def nan_in_b(n, dtype):
    off, col, val, b, x0 = ns(n, dtype)
    b[n // 2] = np.nan
    return off, col, val, b, x0


T = gm.TILE
# sizes: 0, 1, 2; one workgroup with every n mod V (256 .. 259: fewer vectors than lanes too); 2049 / 2051: nine workgroups
SIZES = [Case("n=%d" % n, n, ns, 3, 8) for n in (0, 1, 2, 3, 5, 256, 257, 258, 259, 2049, 2051)]
# restart lengths around the dots' tile, each with at least three cycles begun (2 m + 2 bodies), and 1 and 128
RESTARTS = [Case("restart=%d" % m, 130, skew, m, 2 * m + 2) for m in (1, 2, T - 1, T, T + 1, 2 * T + 1, 128)]
STOPS = [
    # |g_j| < tol inside a cycle (the model's body count k is asserted in the GPU file; check_every 1, 3, 8 and k put it on a batch
    # boundary and inside a replayed batch)
    Case("tol inside a cycle", 25, convdiff5, 30, 200, tol=(1e-4, 1e-10)),
    Case("iter_max inside a cycle and a batch", 259, ns, 4, 11),
    Case("iter_max at a cycle end", 259, ns, 4, 8),
    Case("iter_max on a batch boundary", 259, ns, 5, 16),
]
BREAKDOWNS = [
    Case("breakdown 1: A = 2 I", 5, two_i, 20, 10, tol=(1e-6, 1e-6), exact=True),
    Case("breakdown 1: skew 2 x 2", 2, skew2, 20, 10, tol=(1e-6, 1e-6), exact=True),
    Case("breakdown 2: b = A x0", 2, solved, 20, 10, tol=(1e-6, 1e-6), exact=True),
    Case("breakdown 2 with iter_max 0", 2, solved, 20, 0, tol=(1e-6, 1e-6), exact=True),
    Case("iter_max 0", 259, ns, 20, 0, exact=True),
]
NONFINITE = [Case("NaN in b", 259, nan_in_b, 3, 7, exact=True)]  # (every number of it is NaN: nothing can show)
BIT_CASES = SIZES + RESTARTS + STOPS + BREAKDOWNS + NONFINITE


def big_n(dtype):
    """more than one trip per thread past the grid's cap of 512 workgroups: 2 * 131 072 * V + 3 (tails 3 and 1)"""
    return 2 * 131_072 * vec_len(dtype) + 3
