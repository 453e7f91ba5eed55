"""The right-preconditioned BiCGSTAB (smh_bicgstab_precond_solve*, bicgstab.hip) pinned BIT FOR BIT to tests/pbicgstab_model.py's
"device" mode: x, the number of entered bodies, f64(rr), the breakdown code and `converged` -- f32 and f64, through both entry
points, check_every 1, 3 and 8 -- on the cases of tests/pbicgstab_cases.py.  Jacobi (fused into the solver's sweeps) at the sizes
where each path of the sweeps is first entered, stopping at the full and at the half step, on and inside a replayed batch, on
iter_max, on every breakdown code, from a non-zero x0, on NaN data and through the STREAM, SEQ and AUTO products; SGS and ILU(0) (two
gated triangular applications per body) on convection-diffusion grids in the natural and the red-black ordering, with the node
budget of a captured batch lowered; the statuses, the forwarding of SMH_PRECOND_NONE and the Python class.  The model is fed by the
device's own checked product, as tests/test_pgmres_gpu.py does; tests/test_pbicgstab_model.py shows without a GPU that each case
moves a bit under every wrong variant it can tell apart."""
import ctypes as C
import math

import numpy as np
import pytest

import bicgstab_model as bm
import gmres_cases
import pbicgstab_cases as pc
import pbicgstab_model as pb
import pgmres_model as pm
import sparsemat_amd as sm
import trisolve_model as tm
from kernel_forms import env
from sparsemat_amd import _lib
from test_bicgstab_gpu import assert_result, matrix, results, same, status_of
from test_solver_kernels_gpu import device_product

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
IDS = ["f32", "f64"]
CHECK_EVERY = (1, 3, 8)


def ids(cases):
    return [c.name for c in cases]


def solve_host(a, kind, b, x0, tol, iter_max, variant="seq", factor=None):
    """smh_bicgstab_precond_solve: numpy arrays (check_every is the driver's default, 8)"""
    x = x0.copy()
    s = sm.BiCGStab(tol, iter_max, variant=variant, precond=kind)
    s.solve(a, b, x, factor=factor)
    return results(s, x)


def solve_vec(a, kind, b, x0, tol, iter_max, check_every, variant="seq", factor=None):
    """smh_bicgstab_precond_solve_vec: DenseVec"""
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x0)
    s = sm.BiCGStab(tol, iter_max, variant=variant, check_every=check_every, precond=kind)
    s.solve(a, bd, xd, factor=factor)
    assert same(bd.to_numpy(), b)  # (b is read only)
    return results(s, xd.to_numpy())


class Setup:
    """a case on the device: the handle, ILU's factor (the device's own, asserted to be the model's) and the checked product"""

    def __init__(self, case, dtype, variant="seq"):
        self.case, self.dtype, self.variant = case, dtype, variant
        self.off, self.col, self.val, self.b, self.x0 = case.system(dtype)
        self.a = matrix(self.off, self.col, self.val)
        self.factor = None
        if case.kind == "ilu":
            self.factor, zp = self.a.ilu0()
            assert zp is None and same(self.factor.raw_parts()[2], case.factor(dtype)), "the device's factor is not the model's"
        self.product = device_product(self.a, variant, self.off, self.col, self.val)

    def model(self, **over):
        return self.case.model(self.dtype, product=self.product, **over)

    def args(self, over):
        return over.get("tol", self.case.tol(self.dtype)), over.get("iter_max", self.case.iter_max)

    def host(self, **over):
        return solve_host(self.a, self.case.kind, self.b, self.x0, *self.args(over), self.variant, self.factor)

    def vec(self, check_every, **over):
        return solve_vec(self.a, self.case.kind, self.b, self.x0, *self.args(over), check_every, self.variant, self.factor)

    def check(self, check_every=CHECK_EVERY, **over):
        want = self.model(**over)
        assert_result(self.host(**over), want, (self.case.name, "host", over))
        for ce in check_every:
            assert_result(self.vec(ce, **over), want, (self.case.name, "vec/%d" % ce, over))
        return want


# ---- Jacobi ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", pc.J_SIZES, ids=ids(pc.J_SIZES))
def test_jacobi_bits_at_every_path_size(gpu, dtype, case):
    """n = 0 (one body, r^.v is an empty sum: breakdown 2), 1, 2, 3; 257 .. 264 (every n mod 16 bytes, one workgroup); 2049 / 2051
    (nine workgroups).  8 bodies from a non-zero x0."""
    want = Setup(case, dtype).check()
    if case.n == 0:
        assert (want.iterations, want.breakdown) == (1, 2)
    if case.n > 3:
        assert (want.iterations, want.breakdown, want.converged) == (8, 0, False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_jacobi_bits_past_the_grid_cap(gpu, dtype):
    """gmres_cases.big_n: the grid at its cap of 512 workgroups, a third trip over the 16-byte vectors for a few threads, tails 3
    and 1.  3 bodies."""
    s = Setup(pc.big_n_case(dtype), dtype)
    want = s.model()
    assert (want.iterations, want.breakdown) == (3, 0)
    assert_result(s.vec(3), want, "vec/3")
    assert_result(s.host(), want, "host")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", pc.J_STOPS, ids=ids(pc.J_STOPS))
def test_jacobi_stops_in_exactly_the_stopping_body(gpu, dtype, case):
    """tridiag_ns(259) from x0 = 0: tol 1e-2 stops at the full step of body 10, tol 5e-3 at the half step of body 11.  check_every 1,
    3 and 8 put the body inside a replayed batch, check_every = k on a batch boundary; the stopping body's x update is visible."""
    s = Setup(case, dtype)
    want = s.check()
    k = want.iterations
    assert (k, want.half_step, want.converged, want.breakdown) == ((11, True, True, 0) if "half" in case.name else (10, False, True, 0))
    assert not same(want.x, s.model(tol=0.0, iter_max=k - 1).x)
    assert_result(s.vec(k), want, "a batch boundary")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_jacobi_iter_max_ends_the_loop(gpu, dtype):
    """tol = 0 on tridiag_ns(259): iter_max 11 (inside a batch of 3 and of 8); iter_max 0 leaves x0 and reports the initial r.r."""
    inside, zero = pc.J_ITER_MAX
    want = Setup(inside, dtype).check()
    assert (want.iterations, want.breakdown, want.converged) == (11, 0, False)
    s = Setup(zero, dtype)
    want = s.check(check_every=(0, 2))
    assert (want.iterations, want.breakdown) == (0, 0) and same(want.x, s.x0) and want.r_norm_squared > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_jacobi_exact_cases(gpu, dtype):
    """A = diag(2^k), b = 3 e_3: one body, v = r, alpha = 1, s = 0: the half-step stop with tol > 0, breakdown 3 with tol = 0, x = 3 / d_3
    e_3 either way.  Breakdown 1 worked by hand (pbicgstab_cases.hand_2x2).  Breakdown 2: b = 0.  NaN in b: no stop, no breakdown,
    all 7 bodies."""
    stop, b3, b1, b2, nan = pc.J_EXACT
    want = Setup(stop, dtype).check(check_every=(0, 2))
    assert (want.iterations, want.breakdown, want.half_step, want.r_norm_squared) == (1, 0, True, 0.0) and want.x.tolist() == [0, 0, 0, 1.5, 0, 0, 0]
    want = Setup(b3, dtype).check(check_every=(0, 2))
    assert (want.iterations, want.breakdown, want.r_norm_squared) == (1, 3, 0.0) and want.x.tolist() == [0, 0, 0, 1.5, 0, 0, 0]
    want = Setup(b1, dtype).check(check_every=(0, 2))
    assert (want.iterations, want.breakdown, want.r_norm_squared) == (1, 1, 1.25) and want.x.tolist() == [-0.5, 0.125]
    want = Setup(b2, dtype).check(check_every=(0, 2))
    assert (want.iterations, want.breakdown, want.r_norm_squared) == (1, 2, 0.0) and not want.x.any()
    want = Setup(nan, dtype).check()
    assert (want.iterations, want.breakdown) == (7, 0) and np.isnan(want.x).all() and math.isnan(want.r_norm_squared)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_jacobi_stream_seq_and_auto_products(gpu, dtype):
    """tridiag_ns(259), 11 bodies from a random x0 through the three products; the model takes each from the device."""
    case = pc.J_ITER_MAX[0]
    for variant in ("stream", "seq", "auto"):
        s = Setup(case, dtype, variant)
        want = s.model()
        assert (want.iterations, want.breakdown) == (11, 0)
        assert_result(s.host(), want, (variant, "host"))
        assert_result(s.vec(3), want, (variant, "vec/3"))


# ---- SGS and ILU(0) --------------------------------------------------------------------------------------------------------------
TRI = pc.SGS + pc.ILU


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", TRI, ids=ids(TRI))
def test_triangular_kinds_equal_the_model(gpu, dtype, case):
    """convdiff2d(12, 1.0) and (24, 1.0): the rows as built (SGS), sorted, and red-black permuted.  5 bodies from a random x0
    (iter_max inside a batch of 3 and of 8); from x0 = 0 to tol (5 to 23 bodies, at the half and at the full step; the stop inside a
    batch, and with check_every = k on its boundary)."""
    s = Setup(case, dtype)
    g = int(round(math.sqrt(case.n)))
    lv = (s.factor or s.a).trisolve_levels("lower")
    if "red_black" in case.name:  # two levels of g g / 2 rows: 72 share one single-workgroup launch, 288 are a launch each
        assert lv["n_levels"] == 2 and lv["n_launches"] == (1 if g == 12 else 2) and lv["small_level_rows"] == 128
    else:  # many small levels: one single-workgroup launch
        assert lv["n_levels"] == 2 * g - 1 and lv["n_launches"] == 1
    want = s.check()
    if case.iter_max == 5:
        assert (want.iterations, want.breakdown, want.converged) == (5, 0, False)
    else:
        k = want.iterations
        assert 5 <= k <= 23 and want.converged and want.breakdown == 0 and not same(want.x, s.model(tol=0.0, iter_max=k - 1).x)
        assert_result(s.vec(k), want, (case.name, "a batch boundary"))
        r = s.b.astype(np.longdouble) - s.product(want.x).astype(np.longdouble)
        assert float(np.sqrt(np.sum(r * r))) < 2 * case.tol(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["sgs", "ilu"])
def test_node_budget_changes_no_bit(gpu, kind, dtype):
    """The red-black 24 x 24 grid: 2 launches per solve, 4 per application, 8 + 8 + 9 nodes per body.  With the budget of a captured
    batch lowered to 100 nodes (SMH_SGS_GRAPH_NODES) batches of 8 bodies become batches of 4; lowered to 8 a single body is beyond
    it and the loop runs uncaptured.  Both give the bits of the replayed route, on iter_max and on a stop on tol."""
    cases = [c for c in (pc.SGS if kind == "sgs" else pc.ILU) if "(24, 1.0) red_black" in c.name]
    assert len(cases) == 2
    for case in cases:
        s = Setup(case, dtype)
        want = s.model()
        for nodes in (None, "100", "8"):
            with env(SMH_SGS_GRAPH_NODES=nodes):
                assert_result(s.vec(8), want, (case.name, "budget", nodes))
                assert_result(s.host(), want, (case.name, "budget, host", nodes))


# ---- forwarding, the Python class, reproducibility, the statuses ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_precond_none_is_bicgstab_bit_for_bit(gpu, dtype):
    """SMH_PRECOND_NONE through both new entry points: the outputs of smh_bicgstab_solve*, and bicgstab_model's."""
    off, col, val, b, x0 = gmres_cases.ns(259, dtype)
    a = matrix(off, col, val)
    want = bm.bicgstab(off, col, val, b, x0, 0.0, 11)
    L = sm.lib()
    outs = lambda: (C.c_size_t(), C.c_double(), C.c_int())
    var = _lib.VARIANTS["seq"]
    x, o = x0.copy(), outs()
    _lib.check(L.smh_bicgstab_precond_solve(a._h, _lib.SMH_PRECOND_NONE, None, b.ctypes.data, 259, x.ctypes.data, 259, 0.0, 11, var, *map(C.byref, o)))
    assert_result((x, o[0].value, o[1].value, o[2].value, False), want, "host")
    bd, xd, o = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x0), outs()
    _lib.check(L.smh_bicgstab_precond_solve_vec(a._h, _lib.SMH_PRECOND_NONE, None, bd._h, xd._h, 0.0, 11, var, 3, *map(C.byref, o)))
    assert_result((xd.to_numpy(), o[0].value, o[1].value, o[2].value, False), want, "vec")
    plain = sm.BiCGStab(0.0, 11, variant="seq")
    x2 = x0.copy()
    plain.solve(a, b, x2)
    assert same(x2, x) and plain.precond is None


def test_python_class_factors_by_itself(gpu):
    """precond="ilu" with factor=None calls mat.ilu0(): the bits of a passed factor; `factor` and `zero_pivot` are left behind."""
    case = pc.ILU[1]
    s = Setup(case, F64)
    want = s.model()
    own = sm.BiCGStab(case.tol(F64), case.iter_max, variant="seq", precond="ilu")
    x = s.x0.copy()
    own.solve(s.a, s.b, x)
    assert_result(results(own, x), want, "factor=None")
    assert own.zero_pivot is None and same(own.factor.raw_parts()[2], case.factor(F64))
    own.solve(s.a, s.b, s.x0.copy(), factor=s.factor)
    assert own.factor is s.factor and own.zero_pivot is None and own.iterations == want.iterations
    # a factor whose factorization met a zero pivot is reported, and refused by the solve (a zero diagonal entry)
    sing = matrix(*tm.from_rows([[(0, 1), (1, 1)], [(0, 1), (1, 1)]], F64))
    st, msg = status_of(lambda: own.solve(sing, np.ones(2), np.zeros(2)))
    assert st == _lib.SMH_ERR_INVALID and "row 1" in msg and "ILU" in msg and own.zero_pivot == 1


def test_solves_are_reproducible(gpu):
    """two runs of every kind give the same bytes"""
    for case in (pc.J_SIZES[-1], pc.SGS[-1], pc.ILU[-1]):
        s = Setup(case, F32)
        first, again = s.vec(8), s.vec(8)
        assert first[0].tobytes() == again[0].tobytes() and first[1:] == again[1:], case.name


def test_statuses_leave_x_untouched(gpu):
    f = F64
    L = sm.lib()
    off, col, val = pm.sort_rows(*bm.convdiff2d(5, 1.0, f))
    n = 25
    a = matrix(off, col, val)
    fac, _ = a.ilu0()
    b, x = np.ones(n, f), np.full(n, 7.0)
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x)
    solver = lambda kind: sm.BiCGStab(1e-10, 50, variant="seq", precond=kind)
    wide = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 2], np.ones(2, f))
    for kind in pc.KINDS:
        s = solver(kind)
        factor = fac if kind == "ilu" else None
        # smh_bicgstab_solve's: not square, the lengths, b and x the same storage, a DenseVec of the other dtype, NULL vectors
        wf = matrix([0, 1, 2], [0, 1], np.ones(2, f)) if kind == "ilu" else None
        assert status_of(lambda: s.solve(wide, np.ones(2, f), np.full(2, 7.0), factor=wf))[0] == _lib.SMH_ERR_NOT_SQUARE
        assert status_of(lambda: s.solve(a, np.ones(n - 1, f), x, factor=factor))[0] == _lib.SMH_ERR_DIM_MISMATCH
        assert status_of(lambda: s.solve(a, b, np.full(n - 1, 7.0), factor=factor))[0] == _lib.SMH_ERR_DIM_MISMATCH
        assert status_of(lambda: s.solve(a, sm.DenseVec.from_vec(np.ones(n + 1, f)), xd, factor=factor))[0] == _lib.SMH_ERR_DIM_MISMATCH
        assert status_of(lambda: s.solve(a, xd, xd, factor=factor))[0] == _lib.SMH_ERR_INVALID
        assert status_of(lambda: s.solve(a, x, x, factor=factor))[0] == _lib.SMH_ERR_INVALID
        assert status_of(lambda: s.solve(a, sm.DenseVec.from_vec(np.ones(n, F32)), xd, factor=factor))[0] == _lib.SMH_ERR_INVALID
        code, fh = _lib.PRECONDS[kind], factor._h if factor else None
        assert L.smh_bicgstab_precond_solve(a._h, code, fh, None, n, x.ctypes.data, n, 1e-10, 5, 0, None, None, None) == _lib.SMH_ERR_INVALID
        assert L.smh_bicgstab_precond_solve_vec(a._h, code, fh, None, xd._h, 1e-10, 5, 0, 0, None, None, None) == _lib.SMH_ERR_INVALID
        assert L.smh_bicgstab_precond_solve(None, code, fh, b.ctypes.data, n, x.ctypes.data, n, 1e-10, 5, 0, None, None, None) == _lib.SMH_ERR_INVALID
        assert s.iterations is None and s.breakdown is None  # (a refused call reports nothing)
    # precond and f: a kind out of range, a factor with another kind, ILU without one
    for code, fh in ((4, None), (-1, None), (_lib.SMH_PRECOND_NONE, fac._h), (_lib.SMH_PRECOND_JACOBI, fac._h), (_lib.SMH_PRECOND_SGS, fac._h),
                     (_lib.SMH_PRECOND_ILU, None)):
        assert L.smh_bicgstab_precond_solve(a._h, code, fh, b.ctypes.data, n, x.ctypes.data, n, 1e-10, 5, 0, None, None, None) == _lib.SMH_ERR_INVALID
        assert L.smh_bicgstab_precond_solve_vec(a._h, code, fh, bd._h, xd._h, 1e-10, 5, 0, 0, None, None, None) == _lib.SMH_ERR_INVALID
    assert status_of(lambda: solver("sgs").solve(a, b, x, factor=fac))[0] == _lib.SMH_ERR_INVALID
    # ILU: what smh_pcg_ilu_solve decides about f -- n, dtype, an orphaned entry, a zero and an absent diagonal entry (the row named)
    ilu = solver("ilu")
    small = matrix(*pm.sort_rows(*bm.convdiff2d(4, 1.0, f))).ilu0()[0]
    assert status_of(lambda: ilu.solve(a, b, x, factor=small))[0] == _lib.SMH_ERR_DIM_MISMATCH
    assert status_of(lambda: ilu.solve(a, bd, xd, factor=small))[0] == _lib.SMH_ERR_DIM_MISMATCH
    w = fac.raw_parts()[2]
    assert status_of(lambda: ilu.solve(a, b, x, factor=matrix(off, col, w.astype(F32))))[0] == _lib.SMH_ERR_INVALID
    orphan = sm.SparseMatCRS.from_triplets([1, 0, 1, 0], [1, 0, 0, 1], np.ones(4, f), into_crs=True)
    two = matrix([0, 2, 4], [0, 1, 0, 1], np.array([4.0, 1, 1, 4]))
    assert orphan.orphans() == 1
    st, msg = status_of(lambda: ilu.solve(two, np.ones(2), np.full(2, 7.0), factor=orphan))
    assert st == _lib.SMH_ERR_INVALID and "orphan" in msg
    pos = tm.diag_positions(off, col)
    w0 = w.copy()
    w0[pos[13]] = 0.0  # a zero-pivot factor
    st, msg = status_of(lambda: ilu.solve(a, b, x, factor=matrix(off, col, w0)))
    assert st == _lib.SMH_ERR_INVALID and "row 13" in msg and "ILU" in msg
    keep = np.ones(len(col), bool)
    keep[pos[[9, 17]]] = False
    o2 = np.zeros(n + 1, np.uint32)
    o2[1:] = np.cumsum(np.add.reduceat(keep.astype(np.int64), off[:-1].astype(np.int64)))
    st, msg = status_of(lambda: ilu.solve(a, bd, xd, factor=matrix(o2, col[keep], w[keep])))
    assert st == _lib.SMH_ERR_INVALID and "row 9" in msg
    # SGS and Jacobi: a zero or absent diagonal entry of the matrix, the row named; SGS: an orphaned entry, a stored column >= n
    v0 = val.copy()
    v0[pos[13]] = 0.0
    for kind, word in (("sgs", "SGS"), ("jacobi", "Jacobi")):
        st, msg = status_of(lambda: solver(kind).solve(matrix(off, col, v0), b, x))
        assert st == _lib.SMH_ERR_INVALID and "row 13" in msg and word in msg, (kind, msg)
        st, msg = status_of(lambda: solver(kind).solve(matrix(o2, col[keep], val[keep]), bd, xd))
        assert st == _lib.SMH_ERR_INVALID and "row 9" in msg, (kind, msg)
    st, msg = status_of(lambda: solver("sgs").solve(orphan, np.ones(2), np.full(2, 7.0)))
    assert st == _lib.SMH_ERR_INVALID and "orphan" in msg
    beyond = sm.SparseMatCRS.from_raw_parts(2, 2, [0, 1, 3], [0, 1, 5], np.ones(3, f), validate=False)
    assert status_of(lambda: solver("sgs").solve(beyond, np.ones(2), np.full(2, 7.0)))[0] == _lib.SMH_ERR_INDEX_RANGE
    assert x.tolist() == [7.0] * n and xd.to_numpy().tolist() == [7.0] * n
    # ... and the output pointers may be NULL
    assert L.smh_bicgstab_precond_solve_vec(a._h, _lib.SMH_PRECOND_ILU, fac._h, bd._h, xd._h, 1e-10, 50, _lib.VARIANTS["seq"], 0, None, None, None) == 0
    want = pb.pbicgstab(off, col, val, b, x, 1e-10, 50, pm.ilu(off, col, w))
    assert same(xd.to_numpy(), want.x)
