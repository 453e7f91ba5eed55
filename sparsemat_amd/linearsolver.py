"""ConjugateGradient: host-side mirror of the reference's ``LinearSolver`` / ``ConjugateGradient``
(linearsolver.rs:6-61).

* ``ConjugateGradient``     -- one GPU: the whole iteration runs device-resident inside the HIP library
                               (``smh_cg_solve*``: fused kernels, scalars in HBM, hipGraph replay).
* ``ParConjugateGradient``  -- the same recurrence over a row-partitioned ``SparseMatPar`` (one process per
                               GPU): per iteration one halo exchange of p, the local SpMV, and TWO scalar
                               all-reduces (p.Ap and r.r) on device-resident 1-element tensors; the vector
                               updates are the library's kernels with device-resident scalars
                               (``smh_blas_*_dev``), so no scalar visits the host except the stop test.
* ``SGSConjugateGradient``  -- an extension: CG preconditioned by symmetric Gauss-Seidel through two level-scheduled sparse
                               triangular solves (``smh_pcg_sgs_solve*``), device-resident like ``ConjugateGradient``.
* ``ILUConjugateGradient``  -- an extension: CG preconditioned by ILU(0) (``SparseMatCRS.ilu0``, ``smh_pcg_ilu_solve*``): the same two
                               solves on a factor computed on the device.
* ``FSAIConjugateGradient`` -- an extension: CG preconditioned by the factorized sparse approximate inverse (``SparseMatCRS.fsai``,
                               ``smh_pcg_fsai_solve*``): z = G^T (G r) by two products.
* ``BiCGStab``              -- an extension for non-symmetric systems: the stabilised bi-conjugate gradient recurrence,
                               device-resident like ``ConjugateGradient`` (``smh_bicgstab_solve*``).  ``precond="jacobi"``,
                               ``"sgs"`` or ``"ilu"``: right-preconditioned (``smh_bicgstab_precond_solve*``).
* ``GMRES``                 -- an extension for non-symmetric systems: restarted GMRES(m), the robust companion of ``BiCGStab``
                               (``smh_gmres_solve*``); its Krylov basis stays on the device.  ``precond="jacobi"``, ``"sgs"`` or
                               ``"ilu"``: right-preconditioned (``smh_gmres_precond_solve*``).
* ``IterativeRefinement``   -- an extension: an f64 answer from f32 solves (``smh_refine_solve*``): the residual in f64, the correction
                               by one of the solvers above on an f32 copy of the matrix, the update in f64.
"""
import math

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .densevec import DenseVec
from .multivec import MultiVec, pack_host


class _DeviceSolver:
    """What the device-resident solvers share: the settings, the results of the last solve, and the one call into the library."""

    def __init__(self, tol=1e-12, iter_max=10_000, variant="auto", check_every=0):
        self.tol = float(tol)
        self.iter_max = int(iter_max)
        self.variant = variant
        self.check_every = int(check_every)
        self.iterations = None  # loop bodies entered by the last solve
        self.r_norm_squared = None  # last r.r (as f64)
        self.graph_replays = None  # batches the last solve replayed from its captured graph (0: launched one by one, _solve)

    def _solve(self, vec_fn, host_fn, mat, b, x, handles=(), extra_out=(), extra_in=()):
        """Two ``DenseVec``s go to ``vec_fn`` (None: the solver has no such form), anything else to ``host_fn`` as an array-like b and
        a contiguous numpy x of the matrix dtype, updated in place.  ``handles``: what the call takes after the matrix;
        ``extra_out``: ctypes out-parameters after iters and rr; ``extra_in``: what the call takes after iter_max.  Sets ``iterations`` and ``r_norm_squared``."""
        iters, rr = C.c_size_t(), C.c_double()
        out = [C.byref(iters), C.byref(rr)] + [C.byref(o) for o in extra_out]
        var = _lib.VARIANTS[self.variant]
        if vec_fn is not None and isinstance(b, DenseVec) and isinstance(x, DenseVec):
            check(vec_fn(mat._h, *handles, b._h, x._h, self.tol, self.iter_max, *extra_in, var, self.check_every, *out))
        else:
            if not (isinstance(x, np.ndarray) and x.dtype == mat.dtype and x.flags.c_contiguous):
                raise TypeError("x must be a contiguous numpy array of the matrix dtype (updated in place)")
            bb = np.ascontiguousarray(b, dtype=mat.dtype)
            check(host_fn(mat._h, *handles, bb.ctypes.data if bb.size else None, bb.size, x.ctypes.data if x.size else None, x.size,
                          self.tol, self.iter_max, *extra_in, var, *out))
        self.iterations, self.r_norm_squared, self.graph_replays = iters.value, rr.value, lib().smh_last_solve_replays()
        return x


class ConjugateGradient(_DeviceSolver):
    """``ConjugateGradient::default()`` == ``ConjugateGradient()`` (tol 1e-12, iter_max 10000,
    linearsolver.rs:17-24).  The reference keeps both fields private; ``new(tol, iter_max)`` is the
    documented addition."""

    @classmethod
    def default(cls):
        return cls()

    @classmethod
    def new(cls, tol, iter_max):
        return cls(tol, iter_max)

    def solve(self, mat, b, x):
        """LinearSolver::solve(&self, mat, b, x): x is updated in place (linearsolver.rs:27-61).
        Raises SparseMatPanic("Matrix is not symmetric") / ("Matrix and vector size mismatch")."""
        return self._solve(lib().smh_cg_solve_vec, lib().smh_cg_solve, mat, b, x)

    def solve_many(self, mat, b, x):
        """``solve`` on k right-hand sides at once (``smh_cg_solve_many``): column c of x is ``solve(mat, b_c, x_c)`` with its
        own alpha, beta, stop test and iteration count; all columns share one sweep over the matrix per body.  Two
        ``MultiVec``s, or a ``(k, n)`` array-like b with a contiguous ``(k, n)`` numpy x of the matrix dtype; x is updated in
        place.  Afterwards ``iterations`` is an integer array of k and ``r_norm_squared`` an f64 array of k.  Same panics
        as ``solve``."""
        if isinstance(b, MultiVec) and isinstance(x, MultiVec):
            k = b.count()
            iters, rr = np.zeros(max(k, 1), np.uintp), np.zeros(max(k, 1), np.float64)
            check(lib().smh_cg_solve_many(mat._h, b._h, x._h, self.tol, self.iter_max, self.check_every,
                                          iters.ctypes.data_as(C.POINTER(C.c_size_t)), rr.ctypes.data_as(C.POINTER(C.c_double))))
        else:
            if not (isinstance(x, np.ndarray) and x.dtype == mat.dtype and x.flags.c_contiguous and x.ndim == 2):
                raise TypeError("x must be a contiguous (k, n) numpy array of the matrix dtype (updated in place)")
            bb = pack_host(b, mat.dtype)
            if bb.shape != x.shape:
                raise _lib.SparseMatPanic(_lib.SMH_ERR_DIM_MISMATCH, "Matrix and vector size mismatch")
            k, n = x.shape
            iters, rr = np.zeros(max(k, 1), np.uintp), np.zeros(max(k, 1), np.float64)
            check(lib().smh_cg_solve_many_host(mat._h, bb.ctypes.data if bb.size else None, n, k, x.ctypes.data if x.size else None,
                                               self.tol, self.iter_max, iters.ctypes.data_as(C.POINTER(C.c_size_t)),
                                               rr.ctypes.data_as(C.POINTER(C.c_double))))
        self.iterations, self.r_norm_squared = iters[:k].astype(np.int64), rr[:k]
        return x


class JacobiConjugateGradient(_DeviceSolver):
    """Jacobi-preconditioned CG -- an EXTENSION (the reference has no preconditioner): the
    recurrence of ``ConjugateGradient::solve`` with z = r / diag(A); same guards, stop rule and panics
    (``smh_pcg_jacobi_solve``).  Host vectors; x (numpy array of the matrix dtype) is updated in place."""

    def __init__(self, tol=1e-12, iter_max=10_000, variant="auto"):
        super().__init__(tol, iter_max, variant)
        del self.check_every  # (the library's Jacobi-PCG takes none)

    def solve(self, mat, b, x):
        return self._solve(None, lib().smh_pcg_jacobi_solve, mat, b, x)


class SGSConjugateGradient(_DeviceSolver):
    """CG preconditioned by symmetric Gauss-Seidel, M = (D + L) D^-1 (D + U) -- an EXTENSION: the recurrence of
    ``JacobiConjugateGradient`` with z = M^-1 r by two level-scheduled sparse triangular solves (``smh_pcg_sgs_solve*``); same
    guards, stop rule and panics, device-resident like ``ConjugateGradient``.  The number of levels -- hence of kernel launches
    per body -- follows the ordering of the matrix (``SparseMatCRS.trisolve_levels``): a red-black or multicolour numbering
    (``permute_symmetric``) has few.  x is updated in place: two ``DenseVec``s, or an array-like b with a contiguous numpy x."""

    def solve(self, mat, b, x):
        return self._solve(lib().smh_pcg_sgs_solve_vec, lib().smh_pcg_sgs_solve, mat, b, x)


class ILUConjugateGradient(_DeviceSolver):
    """CG preconditioned by the incomplete LU factorization without fill, M = L U (``SparseMatCRS.ilu0``) -- an EXTENSION: the
    recurrence of ``SGSConjugateGradient`` with z = U^-1 L^-1 r by a unit-lower and an upper triangular solve on the factor
    (``smh_pcg_ilu_solve*``); the product is the matrix's.  ``solve(mat, b, x, factor=None)`` factors ``mat`` itself when no factor
    is given (afterwards ``factor`` holds the one used and ``zero_pivot`` what its factorization reported, None for a passed
    factor).  x is updated in place: two ``DenseVec``s, or an array-like b with a contiguous numpy x."""

    def __init__(self, tol=1e-12, iter_max=10_000, variant="auto", check_every=0):
        super().__init__(tol, iter_max, variant, check_every)
        self.factor = None
        self.zero_pivot = None

    def solve(self, mat, b, x, factor=None):
        self.zero_pivot = None
        if factor is None:
            factor, self.zero_pivot = mat.ilu0()
        self.factor = factor
        return self._solve(lib().smh_pcg_ilu_solve_vec, lib().smh_pcg_ilu_solve, mat, b, x, handles=(factor._h,))


class FSAIConjugateGradient(_DeviceSolver):
    """CG preconditioned by the factorized sparse approximate inverse, M^-1 = G^T G (``SparseMatCRS.fsai``) -- an EXTENSION: the
    recurrence of ``SGSConjugateGradient`` with z = G^T (G r) by two products on the factor handles (``smh_pcg_fsai_solve*``) -- no
    schedule, no levels, the same cost in every ordering; the body's own product is the matrix's.  ``factor``: a pair ``(g, gt)``,
    given here or to ``solve``; without one ``solve`` factors ``mat`` itself and raises ValueError when the factorization reports a
    row that is not positive definite (afterwards ``factor`` holds the pair used and ``not_spd`` what its factorization reported,
    None for a passed pair).  x is updated in place: two ``DenseVec``s, or an array-like b with a contiguous numpy x."""

    def __init__(self, tol=1e-12, iter_max=10_000, factor=None, variant="auto", check_every=0):
        super().__init__(tol, iter_max, variant, check_every)
        self.factor = factor
        self.not_spd = None
        self._given = factor

    def solve(self, mat, b, x, factor=None):
        self.not_spd = None
        factor = factor if factor is not None else self._given
        if factor is None:
            g, gt, self.not_spd = mat.fsai()
            if self.not_spd is not None:
                raise ValueError("FSAI: the matrix is not positive definite (row %d)" % self.not_spd)
            factor = (g, gt)
        self.factor = factor
        return self._solve(lib().smh_pcg_fsai_solve_vec, lib().smh_pcg_fsai_solve, mat, b, x, handles=(factor[0]._h, factor[1]._h))


class _RightPreconditioned(_DeviceSolver):
    """What ``BiCGStab`` and ``GMRES`` share: ``precond``, and what a solve makes of it and of ``factor``."""

    _entry = None  # the stem of the library's entry points: "smh_bicgstab", "smh_gmres"

    def __init__(self, tol, iter_max, variant, check_every, precond):
        super().__init__(tol, iter_max, variant, check_every)
        if precond not in _lib.PRECOND_NAMES:
            raise ValueError('precond must be None, "jacobi", "sgs", "ilu" or "fsai"')
        self.precond = precond
        self.breakdown = None
        self.factor = None
        self.zero_pivot = None
        self.singular = None

    def _resolve(self, mat, factor):
        """``(vec_fn, host_fn, handles)`` of a solve on ``mat``: the pair of entry points -- the plain one, ``_fsai_``'s or
        ``_precond_``'s -- and what they take after the matrix.  Without a factor "ilu" factors ``mat`` through ``ilu0`` and "fsai"
        through ``fsai_ns``; ``factor``, ``zero_pivot`` and ``singular`` are set as the classes' docstrings say."""
        def entry(kind):
            return getattr(lib(), "%s_%ssolve_vec" % (self._entry, kind)), getattr(lib(), "%s_%ssolve" % (self._entry, kind))

        if self.precond is None and factor is None:
            return entry("") + ((),)
        if self.precond == "fsai":
            self.singular = None
            if factor is None:
                gl, gu, self.singular = mat.fsai_ns()
                factor = (gl, gu)
            self.factor = factor
            return entry("fsai_") + ((factor[0]._h, factor[1]._h),)
        self.zero_pivot = None
        if self.precond == "ilu" and factor is None:
            factor, self.zero_pivot = mat.ilu0()
        self.factor = factor
        return entry("precond_") + ((_lib.PRECONDS[self.precond], factor._h if factor is not None else None),)


class BiCGStab(_RightPreconditioned):
    """BiCGSTAB (van der Vorst, unpreconditioned) for non-symmetric systems -- an EXTENSION (the reference's only solver is the
    conjugate gradient): device-resident like ``ConjugateGradient``, the same guards, panics and stop rule
    (``sqrt(f64(r.r)) < tol`` after the update of r, and on ``s.s`` at the half step), ``smh_bicgstab_solve*``.

    After ``solve``: ``iterations`` (bodies entered), ``r_norm_squared`` (the last r.r, or s.s after a half-step stop, as
    f64), ``breakdown`` (0 none; 1 rho' == 0 or omega == 0: x keeps that body's update; 2 r^.v == 0: x untouched by that body;
    3 t.t == 0: x has taken p*alpha) and ``converged`` (a stop test ended the loop: neither a breakdown nor iter_max).

    ``precond``: None, "jacobi", "sgs" or "ilu" -- RIGHT preconditioning (``smh_bicgstab_precond_solve*``): A M^-1 u = b,
    x = M^-1 u, so the residual the recurrence carries is the true one and the stop rule, ``r_norm_squared`` and ``breakdown`` keep
    their meaning (in the lines above x takes M^-1 p and M^-1 s where it took p and s).  M^-1 is applied twice per body: a division
    by the diagonal fused into the solver's sweeps ("jacobi"), or ``SparseMatCRS.sgs_apply`` / ``ilu_apply``'s two level-scheduled
    triangular solves ("sgs" on the matrix, "ilu" on a factor).  ``solve(mat, b, x, factor=None)`` with "ilu" factors ``mat`` itself
    when no factor is given (afterwards ``factor`` holds the one used and ``zero_pivot`` what its factorization reported, None for a
    passed factor).

    ``precond="fsai"`` (``smh_bicgstab_fsai_solve*``): M^-1 v = gt (g v) by two products on a pair of handles, ``factor=(g, gt)`` --
    ``SparseMatCRS.fsai_ns``'s (G_L, G_U), or ``fsai``'s (G, G^T) for a symmetric matrix; no schedule, no levels, the same cost in every
    ordering.  Without a factor ``solve`` factors ``mat`` through ``fsai_ns`` (afterwards ``factor`` holds the pair used and
    ``singular`` what the factorization reported, None for a passed pair)."""

    _entry = "smh_bicgstab"

    def __init__(self, tol=1e-12, iter_max=10_000, variant="auto", check_every=0, precond=None):
        super().__init__(tol, iter_max, variant, check_every, precond)
        self.converged = None

    def solve(self, mat, b, x, factor=None):
        """x is updated in place: two ``DenseVec``s, or an array-like b with a contiguous numpy x of the matrix dtype.  Raises
        SparseMatPanic("Matrix is not symmetric") for a matrix that is not square / ("Matrix and vector size mismatch")."""
        brk = C.c_int()
        vec_fn, host_fn, handles = self._resolve(mat, factor)
        self._solve(vec_fn, host_fn, mat, b, x, handles=handles, extra_out=(brk,))
        self.breakdown = brk.value
        # every entered body that ends without a breakdown has tested the r.r it reports: under tol means that test stopped the loop
        self.converged = self.breakdown == 0 and self.iterations > 0 and math.sqrt(self.r_norm_squared) < self.tol
        return x


class GMRES(_RightPreconditioned):
    """Restarted GMRES(m) (Saad & Schultz, unpreconditioned) for non-symmetric systems -- an EXTENSION, the robust companion of
    ``BiCGStab``: it cannot break down before the Krylov space is exhausted and does not stagnate on a spectrum near the
    imaginary axis; a body is one product and sweeps over a device-resident basis of up to ``restart`` + 1 vectors
    (``smh_gmres_solve*``).  ``restart``: 1 .. 128 (0: the library's default, 30).  Same guards and panics as ``BiCGStab``.

    After ``solve``: ``iterations`` (bodies entered), ``r_norm_squared`` (the r.r of the residual rebuilt from the basis at the
    last cycle end -- no product is spent on it --, the initial residual's before the first; as f64), ``cycles`` (the number of
    times a v_0 was formed) and ``breakdown`` (0 none; 1 the Krylov space is exhausted: x is updated from it; 2 the residual
    at a cycle's start is exactly zero: x is the solution as it stands).

    ``precond``: None, "jacobi", "sgs" or "ilu" -- RIGHT preconditioning (``smh_gmres_precond_solve*``): A M^-1 u = b, x = M^-1 u,
    so the residual GMRES minimises is the true one and the stop rule, ``r_norm_squared``, ``cycles`` and ``breakdown`` keep their
    meaning.  M^-1 is applied once per body and once per cycle end: a division by the diagonal fused into the solver's sweeps
    ("jacobi"), or ``SparseMatCRS.sgs_apply`` / ``ilu_apply``'s two level-scheduled triangular solves ("sgs" on the matrix, "ilu" on
    a factor).  ``solve(mat, b, x, factor=None)`` with "ilu" factors ``mat`` itself when no factor is given (afterwards ``factor``
    holds the one used and ``zero_pivot`` what its factorization reported, None for a passed factor).  ``r_norm_squared`` is the
    RECURRENCE residual's: where the triangular solves amplify rounding (a matrix far from diagonally dominant) it parts from
    |b - A x|^2 -- form that yourself when it matters.

    ``precond="fsai"`` (``smh_gmres_fsai_solve*``): M^-1 v = gt (g v) by two products on a pair of handles, ``factor=(g, gt)`` --
    ``SparseMatCRS.fsai_ns``'s (G_L, G_U), or ``fsai``'s (G, G^T) for a symmetric matrix.  The body's application goes through the
    handles' own kernels; the cycle end's is formed by two storage-order products that run at a cycle end alone.  Without a factor
    ``solve`` factors ``mat`` through ``fsai_ns`` (afterwards ``factor`` holds the pair used and ``singular`` what the factorization
    reported, None for a passed pair)."""

    _entry = "smh_gmres"

    def __init__(self, tol=1e-12, iter_max=10_000, restart=30, variant="auto", check_every=0, precond=None):
        super().__init__(tol, iter_max, variant, check_every, precond)
        self.restart = int(restart)
        self.cycles = None

    def solve(self, mat, b, x, factor=None):
        """x is updated in place: two ``DenseVec``s, or an array-like b with a contiguous numpy x of the matrix dtype.  Raises
        SparseMatPanic("Matrix is not symmetric") for a matrix that is not square / ("Matrix and vector size mismatch")."""
        cycles, brk = C.c_size_t(), C.c_int()
        vec_fn, host_fn, handles = self._resolve(mat, factor)
        self._solve(vec_fn, host_fn, mat, b, x, handles=handles, extra_out=(cycles, brk), extra_in=(self.restart,))
        self.cycles, self.breakdown = cycles.value, brk.value
        return x


class IterativeRefinement:
    """Mixed-precision iterative refinement -- an EXTENSION (``smh_refine_solve*``): an f64-accurate x of A x = b whose bodies run in
    f32.  Each outer step forms r = b - A x in f64, scales it by a power of two to a norm in [1, 2), converts it to f32, solves
    A_lo d = r_lo from d = 0 with the ``inner`` solver ("cg", "bicgstab" or "gmres", preconditioned by ``precond``: None, "jacobi" (not
    with "cg"), "sgs", "ilu" or "fsai") to the absolute tolerance ``inner_tol`` -- a relative reduction of the residual by
    ``inner_tol / 2`` to ``inner_tol`` -- and adds the widened, rescaled d to x in f64: one rounding per element going down and one
    going up.  It stops when sqrt(r.r) < ``tol`` (``code`` 0), after ``outer_max`` steps (1), or when a step does not lower r.r (2:
    the step is undone, x is the better iterate).  ``variant`` is the f64 product's, ``variant_lo`` the inner solver's.

    ``solve(mat, b, x, mat_lo=None, factor=None)``: ``mat`` f64, x updated in place -- two f64 ``DenseVec``s, or an array-like b with a
    contiguous f64 numpy x.  ``mat_lo``: the f32 matrix (None: ``mat.astype(float32)``); ``factor``: the f32 factor of ``mat_lo`` for
    "ilu" (a matrix) or "fsai" (a pair); None factors ``mat_lo`` through ``ilu0``, and through ``fsai`` (inner "cg") or ``fsai_ns``.
    Afterwards ``outer_iterations``, ``iterations`` (the inner solves' bodies in total), ``r_norm_squared`` (the last accepted r.r),
    ``code``, ``mat_lo`` and ``factor`` are set."""

    def __init__(self, tol=1e-12, outer_max=20, inner="cg", precond=None, inner_tol=1e-4, inner_iter_max=10_000, restart=30,
                 variant="auto", variant_lo="auto", check_every=0):
        if inner not in _lib.INNERS:
            raise ValueError('inner must be "cg", "bicgstab" or "gmres"')
        if precond not in _lib.REFINE_PRECONDS:
            raise ValueError('precond must be None, "jacobi", "sgs", "ilu" or "fsai"')
        self.tol, self.outer_max, self.inner, self.precond = float(tol), int(outer_max), inner, precond
        self.inner_tol, self.inner_iter_max, self.restart = float(inner_tol), int(inner_iter_max), int(restart)
        self.variant, self.variant_lo, self.check_every = variant, variant_lo, int(check_every)
        self.outer_iterations = self.iterations = self.r_norm_squared = self.code = None
        self.mat_lo = self.factor = None

    def solve(self, mat, b, x, mat_lo=None, factor=None):
        if mat_lo is None:
            mat_lo = mat.astype(np.float32)
        if factor is None and self.precond == "ilu":
            factor = mat_lo.ilu0()[0]
        elif factor is None and self.precond == "fsai":
            factor = (mat_lo.fsai() if self.inner == "cg" else mat_lo.fsai_ns())[:2]
        self.mat_lo, self.factor = mat_lo, factor
        pair = factor if isinstance(factor, (tuple, list)) else (factor, None)
        handles = [f._h if f is not None else None for f in pair]
        outer, inner, rr, code = C.c_size_t(), C.c_size_t(), C.c_double(), C.c_int()
        head = (mat._h, mat_lo._h, _lib.INNERS[self.inner], _lib.REFINE_PRECONDS[self.precond], handles[0], handles[1])
        tail = (self.tol, self.outer_max, self.inner_tol, self.inner_iter_max, self.restart, _lib.VARIANTS[self.variant],
                _lib.VARIANTS[self.variant_lo], self.check_every, C.byref(outer), C.byref(inner), C.byref(rr), C.byref(code))
        if isinstance(b, DenseVec) and isinstance(x, DenseVec):
            check(lib().smh_refine_solve_vec(*head, b._h, x._h, *tail))
        else:
            if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous):
                raise TypeError("x must be a contiguous f64 numpy array (updated in place)")
            bb = np.ascontiguousarray(b, dtype=np.float64)
            check(lib().smh_refine_solve(*head, bb.ctypes.data if bb.size else None, bb.size, x.ctypes.data if x.size else None, x.size, *tail))
        self.outer_iterations, self.iterations, self.r_norm_squared, self.code = outer.value, inner.value, rr.value, code.value
        return x
