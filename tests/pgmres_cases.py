"""The cases tests/test_pgmres_gpu.py compares bit for bit with pgmres_model's "device" mode -- shared with
tests/test_pgmres_model.py, which shows (without a GPU) that each of them moves a bit under every wrong variant of the arithmetic it
can tell apart.  The builders are gmres_cases' and bicgstab_model's.

Jacobi runs on tridiag_ns (diagonal 2 + c + u_i: a division by it is not a multiplication by its reciprocal); SGS and ILU(0) on
convdiff2d(12, 1.0) and (24, 1.0) in three storage forms: the rows as convdiff2d returns them (diagonal first: unsorted; SGS
alone), sorted ("natural": 2 g - 1 levels of at most g rows -- one single-workgroup launch per solve), and red-black permuted
(reorder_model.permute_symmetric, then sorted: two levels of g g / 2 rows -- 72, and 288 which is past the 128-row switch to the
per-level kernel)."""
import numpy as np

import bicgstab_model as bm
import gmres_cases as gc
import ilu_model as im
import pgmres_model as pm
import reorder_model as rm
import sgs_model as sg

F32, F64 = np.float32, np.float64
KINDS = ("jacobi", "sgs", "ilu")


class Case:
    """kind: the preconditioner; system(dtype) -> (off, col, val, b, x0), computed once; precond(dtype): the model's M^-1 (ILU: on
    the model's factor, which the GPU file asserts to be the device's); exact: every number of the solve is exact in any order, or
    NaN: no wrong variant can show; blind: further variants this case cannot tell apart, with the reason where it is set"""

    def __init__(self, name, kind, n, build, restart, iter_max, tol=(0.0, 0.0), exact=False, blind=()):
        self.name, self.kind, self.n, self.build, self.restart, self.iter_max, self.tols = name, kind, n, build, restart, iter_max, tol
        self.exact, self.blind = exact, tuple(blind)
        self._systems, self._preconds, self._factors = {}, {}, {}

    def system(self, dtype):
        if dtype not in self._systems:
            self._systems[dtype] = self.build(self.n, dtype)
        return self._systems[dtype]

    def tol(self, dtype):
        return self.tols[0] if dtype == F32 else self.tols[1]

    def factor(self, dtype):
        """ilu_model's factor values of the system (ILU cases)"""
        if dtype not in self._factors:
            off, col, val = self.system(dtype)[:3]
            w, zp = im.ilu0(off, col, val, vector=True)
            assert zp is None
            self._factors[dtype] = w
        return self._factors[dtype]

    def precond(self, dtype):
        if dtype not in self._preconds:
            off, col, val = self.system(dtype)[:3]
            self._preconds[dtype] = {"jacobi": lambda: pm.jacobi(off, col, val), "sgs": lambda: pm.sgs(off, col, val),
                                     "ilu": lambda: pm.ilu(off, col, self.factor(dtype))}[self.kind]()
        return self._preconds[dtype]

    def model(self, dtype, product=None, wrong=None, mode="device", **over):
        off, col, val, b, x0 = self.system(dtype)
        tol, iter_max, restart = over.get("tol", self.tol(dtype)), over.get("iter_max", self.iter_max), over.get("restart", self.restart)
        return pm.pgmres(off, col, val, b, x0, tol, iter_max, restart, self.precond(dtype), mode=mode, product=product, wrong=wrong)


# ---- Jacobi -------------------------------------------------------------------------------------------------------------------
def diag_pow2(n, dtype):
    """A = diag(2^k_i) with varying k, b = 3 e_3: v_0 = e_3, u = e_3 / 2, w = A u = e_3 exactly, h = 1, w = 0: one body, hn == 0"""
    d = 2.0 ** (np.arange(n) % 5 - 2)
    off, col, val = np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), d.astype(dtype)
    b = np.zeros(n, dtype)
    b[3] = 3
    return off, col, val, b, np.zeros(n, dtype)


def ns_zero_x0(n, dtype):
    off, col, val, b, x0 = gc.ns(n, dtype)
    return off, col, val, b, np.zeros_like(x0)


def J(name, n, build, restart, iter_max, **kw):
    return Case("jacobi " + name, "jacobi", n, build, restart, iter_max, **kw)


# sizes: 0 .. 3; eight consecutive n around 257 (every n mod 16 bytes in f32, twice over in f64: one workgroup, fewer vectors than
# lanes too); 2049 / 2051: nine workgroups.  GMRES(3), 8 bodies from a non-zero x0, as gmres_cases.SIZES
J_SIZES = [J("n=%d" % n, n, gc.ns, 3, 8) for n in (0, 1, 2, 3, 257, 258, 259, 260, 261, 262, 263, 264, 2049, 2051)]
# restart lengths around the dots' tile and 30, each with three cycles begun (2 m + 2 bodies)
J_RESTARTS = [J("restart=%d" % m, 130, gc.ns, m, 2 * m + 2) for m in (1, 2, gc.T - 1, gc.T, gc.T + 1, 30)]
J_STOPS = [
    J("tol inside a cycle", 259, ns_zero_x0, 30, 200, tol=(1e-2, 1e-2)),  # (body 17 in both precisions: 8.7e-3 after 1.2e-2)
    J("iter_max inside a cycle and a batch", 259, gc.ns, 4, 11),
    J("iter_max at a cycle end", 259, gc.ns, 4, 8),
]
J_SPECIAL = [
    J("breakdown 1: A = diag(d)", 7, diag_pow2, 20, 10, tol=(1e-6, 1e-6), exact=True),
    J("iter_max 0", 259, gc.ns, 20, 0, exact=True),
    J("NaN in b", 259, gc.nan_in_b, 3, 7, exact=True),  # (every number of it is NaN: nothing can show)
]
JACOBI = J_SIZES + J_RESTARTS + J_STOPS + J_SPECIAL


# ---- SGS and ILU(0) -----------------------------------------------------------------------------------------------------------
ORDERINGS = ("unsorted", "natural", "red_black")
_GRIDS = {}


def grid(g, ordering, dtype):
    """(off, col, val, x*) of convdiff2d(g, 1.0) in the ordering; b = A x* is formed on the arrays as stored"""
    key = g, ordering, np.dtype(dtype).name
    if key not in _GRIDS:
        off, col, val = bm.convdiff2d(g, 1.0, dtype)
        x_star = np.random.default_rng(g).uniform(-1, 1, g * g).astype(dtype)
        if ordering != "unsorted":
            off, col, val = pm.sort_rows(off, col, val)
        if ordering == "red_black":
            perm = sg.red_black(g, g)
            off, col, val = pm.sort_rows(*rm.permute_symmetric(g * g, off, col, val, perm))
            x_star = x_star[perm]
        _GRIDS[key] = off, col, val, x_star
    return _GRIDS[key]


def grid_system(g, ordering, random_x0):
    import oracle

    def build(n, dtype):
        off, col, val, x_star = grid(g, ordering, dtype)
        x0 = gc.rhs(n, dtype, g)[1] if random_x0 else np.zeros(n, dtype)
        return off, col, val, oracle.spmv(off, col, val, x_star), x0
    return build


def tri_cases(kind):
    out = []
    for g in (12, 24):
        for ordering in ORDERINGS if kind == "sgs" else ORDERINGS[1:]:
            tag = "%s convdiff2d(%d, 1.0) %s" % (kind, g, ordering)
            # GMRES(5), 12 bodies from a random x0: two restarts, iter_max inside the third cycle (and inside a batch of 8 and of 3)
            out.append(Case(tag + ", restart 5, iter_max 12", kind, g * g, grid_system(g, ordering, True), 5, 12))
            # GMRES(30) from x0 = 0 to the table's tolerances: a stop on tol inside the cycle
            out.append(Case(tag + ", restart 30, to tol", kind, g * g, grid_system(g, ordering, False), 30, 200, tol=(1e-3, 1e-8)))
    return out


SGS = tri_cases("sgs")
ILU = tri_cases("ilu")
BIT_CASES = JACOBI + SGS + ILU


def big_n(dtype):
    return gc.big_n(dtype)
