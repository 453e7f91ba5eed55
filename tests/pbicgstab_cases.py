"""The cases tests/test_pbicgstab_gpu.py compares bit for bit with pbicgstab_model's "device" mode -- shared with
tests/test_pbicgstab_model.py, which shows (without a GPU) that each of them moves a bit under every wrong variant of the arithmetic
it can tell apart.  The builders are pgmres_cases', gmres_cases' and bicgstab_model's.

Jacobi runs on tridiag_ns (diagonal 2 + c + u_i: a division by it is not a multiplication by its reciprocal); SGS and ILU(0) on
convdiff2d(12, 1.0) and (24, 1.0) in pgmres_cases' storage forms: unsorted (SGS alone), natural (one single-workgroup launch per
solve) and red-black (two levels of 72 rows, and of 288: past the 128-row switch to the per-level kernel)."""
import numpy as np

import bicgstab_model as bm
import gmres_cases as gc
import ilu_model as im
import pbicgstab_model as pb
import pgmres_cases as pgc
import pgmres_model as pm

F32, F64 = np.float32, np.float64
KINDS = ("jacobi", "sgs", "ilu")


class Case:
    """kind: the preconditioner; system(dtype) -> (off, col, val, b, x0), computed once; precond(dtype): the model's M^-1 (ILU: on
    the model's factor, which the GPU file asserts to be the device's); exact: every number of the solve is exact in any order, or
    NaN, or no body does arithmetic: no wrong variant can show; blind: {variant: reason} this case cannot tell apart"""

    def __init__(self, name, kind, n, build, iter_max, tol=(0.0, 0.0), exact=False, blind=None):
        self.name, self.kind, self.n, self.build, self.iter_max, self.tols = name, kind, n, build, iter_max, tol
        self.exact, self.blind = exact, dict(blind or {})
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
        tol, iter_max = over.get("tol", self.tol(dtype)), over.get("iter_max", self.iter_max)
        return pb.pbicgstab(off, col, val, b, x0, tol, iter_max, self.precond(dtype), mode=mode, product=product, wrong=wrong)


# ---- Jacobi -------------------------------------------------------------------------------------------------------------------
def J(name, n, build, iter_max, **kw):
    return Case("jacobi " + name, "jacobi", n, build, iter_max, **kw)


def hand_2x2(n, dtype):
    """breakdown 1, worked by hand: d = (2, 4); p^ = (-1, 1/4), v = (-3, 4), rho = 5, rv = 10, alpha = 1/2; s = (-1/2, -1), ss = 5/4;
    s^ = (-1/4, -1/4), t = (1/2, -1/4), ts = 0, omega = 0; x = (-1/2, 1/8), rr = 5/4, rho' = 0"""
    off, col, val = bm.dense_to_crs([[2, -4], [-3, 4]], dtype)
    return off, col, val, np.array([-2, 1], dtype), np.zeros(2, dtype)


def zero_b(n, dtype):
    off, col, val, _, x0 = pgc.ns_zero_x0(n, dtype)
    return off, col, val, np.zeros(n, dtype), x0


# sizes: 0 .. 3; eight consecutive n around 257 (every n mod 16 bytes in f32, twice over in f64: one workgroup, fewer vectors than
# lanes too); 2049 / 2051: nine workgroups.  8 bodies from a non-zero x0 (n <= 3: the model says where the tiny system ends)
J_SIZES = [J("n=%d" % n, n, gc.ns, 8) for n in (0, 1, 2, 3, 257, 258, 259, 260, 261, 262, 263, 264, 2049, 2051)]
# the stops on tridiag_ns(259) from x0 = 0 (the bodies are asserted from the model in both test files): the full step's test, the
# half step's
J_STOPS = [
    J("tol at a full step", 259, pgc.ns_zero_x0, 200, tol=(1e-2, 1e-2)),
    J("tol at a half step", 259, pgc.ns_zero_x0, 200, tol=(5e-3, 5e-3)),
]
J_ITER_MAX = [
    J("iter_max inside a batch", 259, gc.ns, 11),
    J("iter_max 0", 259, gc.ns, 0, exact=True),
]
J_EXACT = [
    J("half-step stop: A = diag(d)", 7, pgc.diag_pow2, 10, tol=(1e-6, 1e-6), exact=True),
    J("breakdown 3: A = diag(d), tol 0", 7, pgc.diag_pow2, 10, exact=True),
    J("breakdown 1: 2 x 2 by hand", 2, hand_2x2, 10, tol=(1e-6, 1e-6), exact=True),
    J("breakdown 2: b = 0", 259, zero_b, 10, tol=(1e-6, 1e-6), exact=True),
    J("NaN in b", 259, gc.nan_in_b, 7, exact=True),  # (every number of it is NaN: nothing can show)
]
JACOBI = J_SIZES + J_STOPS + J_ITER_MAX + J_EXACT


# ---- SGS and ILU(0) -----------------------------------------------------------------------------------------------------------
def tri_cases(kind):
    out = []
    for g in (12, 24):
        for ordering in pgc.ORDERINGS if kind == "sgs" else pgc.ORDERINGS[1:]:
            tag = "%s convdiff2d(%d, 1.0) %s" % (kind, g, ordering)
            out.append(Case(tag + ", iter_max 5", kind, g * g, pgc.grid_system(g, ordering, True), 5))
            out.append(Case(tag + ", to tol", kind, g * g, pgc.grid_system(g, ordering, False), 200, tol=(1e-3, 1e-8)))
    return out


SGS = tri_cases("sgs")
ILU = tri_cases("ilu")
BIT_CASES = JACOBI + SGS + ILU


def big_n_case(dtype):
    """gmres_cases.big_n: the grid at its cap of 512 workgroups, a third trip over the 16-byte vectors for a few threads; 3 bodies"""
    n = gc.big_n(dtype)
    return J("big n", n, lambda n, dt: bm.tridiag_ns(n, 0.5, dt, seed=11) + gc.rhs(n, dt, 11), 3)
