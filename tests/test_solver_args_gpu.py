"""What the entry points of the device-resident solvers answer to arguments they refuse -- the status code and the text of
smh_last_error -- and what ``check_every = 0`` stands for, called through ``_lib.lib()`` as test_cg_many_gpu.py's ``expect`` does.

    vec form:  smh_cg_solve_vec, smh_pcg_sgs_solve_vec, smh_pcg_ilu_solve_vec, smh_bicgstab_solve_vec, smh_cg_solve_many,
               smh_gmres_solve_vec, smh_{gmres,bicgstab}_precond_solve_vec, smh_{pcg,gmres,bicgstab}_fsai_solve_vec
    host form: smh_cg_solve, smh_pcg_jacobi_solve, smh_pcg_sgs_solve, smh_pcg_ilu_solve, smh_bicgstab_solve, smh_cg_solve_many_host,
               smh_gmres_solve, smh_{gmres,bicgstab}_precond_solve, smh_{pcg,gmres,bicgstab}_fsai_solve

A ``_precond_`` entry is a row per kind, "name:none", "name:jacobi", "name:sgs" and "name:ilu".  The tables record what each entry
point does, including where the entry points differ from one another (DESIGN.md lists those differences): ``smh_cg_solve_vec``
words the dtype refusal in its own way and solves with b and x in one storage, of the host forms only BiCGSTAB's and GMRES's refuse
b == x, and ``smh_cg_solve`` leaves the NULL pointer to ``smh_vec_upload``.  Every refusal is decided before any launch: x, iters,
rr, cycles and the breakdown code keep what they held.  The matrices are 2 x 3, 2 x 2 and 3 x 3."""
import ctypes as C

import numpy as np
import pytest

import sparsemat_amd as sm
from sparsemat_amd import _lib

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
OK, DIM, NOT_SQUARE, INVALID = 0, _lib.SMH_ERR_DIM_MISMATCH, _lib.SMH_ERR_NOT_SQUARE, _lib.SMH_ERR_INVALID
SYMMETRIC, SIZE, SAME, NULL_HANDLE = "Matrix is not symmetric", "Matrix and vector size mismatch", "b and x are the same storage", "NULL handle"
VEC_DTYPE = "vector dtype differs from the matrix's"
RESTART = "restart is 129: it must be at most 128 (0: the default, 30)"
TOL, ITER_MAX = 1e-5, 20

# the signature of a host form (its vec form has the same): the handles that follow the matrix ("": none, "f": a factor, "precond":
# the kind and a factor, "pair": g and gt), whether restart follows iter_max, and the out-parameters that follow rr_out
SIG = {"smh_cg_solve": ("", False, ()), "smh_pcg_jacobi_solve": ("", False, ()), "smh_pcg_sgs_solve": ("", False, ()),
       "smh_pcg_ilu_solve": ("f", False, ()), "smh_bicgstab_solve": ("", False, ("brk",)), "smh_gmres_solve": ("", True, ("cycles", "brk")),
       "smh_gmres_precond_solve": ("precond", True, ("cycles", "brk")), "smh_bicgstab_precond_solve": ("precond", False, ("brk",)),
       "smh_pcg_fsai_solve": ("pair", False, ()), "smh_gmres_fsai_solve": ("pair", True, ("cycles", "brk")),
       "smh_bicgstab_fsai_solve": ("pair", False, ("brk",))}
KINDS = ("none", "jacobi", "sgs", "ilu")   # a "name:kind" row calls name with SMH_PRECOND_<kind>
PRECOND = ["smh_gmres_precond_solve", "smh_bicgstab_precond_solve"]
FSAI_HOST = ["smh_pcg_fsai_solve", "smh_gmres_fsai_solve", "smh_bicgstab_fsai_solve"]


def rows(names, suffix="", kinds=KINDS):
    return ["%s%s:%s" % (n, suffix, k) for n in names for k in kinds]


VEC = (["smh_cg_solve_vec", "smh_pcg_sgs_solve_vec", "smh_pcg_ilu_solve_vec", "smh_bicgstab_solve_vec", "smh_cg_solve_many", "smh_gmres_solve_vec"]
       + rows(PRECOND, "_vec") + [n + "_vec" for n in FSAI_HOST])
HOST = (["smh_cg_solve", "smh_pcg_jacobi_solve", "smh_pcg_sgs_solve", "smh_pcg_ilu_solve", "smh_bicgstab_solve", "smh_cg_solve_many_host", "smh_gmres_solve"]
        + rows(PRECOND) + FSAI_HOST)
ILU = ["smh_pcg_ilu_solve_vec", "smh_pcg_ilu_solve"] + rows(PRECOND, "_vec", ("ilu",)) + rows(PRECOND, "", ("ilu",))
FSAI = [n + "_vec" for n in FSAI_HOST] + FSAI_HOST
TRI = ["smh_pcg_sgs_solve_vec", "smh_pcg_sgs_solve"] + rows(PRECOND, "_vec", ("sgs",)) + rows(PRECOND, "", ("sgs",)) + ILU + FSAI
GMRES = [n for n in VEC + HOST if "gmres" in n]
# the host forms that refuse b_host == x_host: BiCGSTAB's and GMRES's, preconditioned or not
HOST_REFUSES_SAME = [n for n in HOST if "bicgstab" in n or "gmres" in n]
DEFAULT_CHECK_EVERY = {n: 4 if n in ("smh_cg_solve_vec", "smh_cg_solve_many") else 8 for n in VEC}
# the vec form that a host form calls or mirrors (smh_pcg_jacobi_solve has none)
VEC_OF = {"smh_cg_solve_many_host": "smh_cg_solve_many"}
VEC_OF.update({n: n.replace("_solve", "_solve_vec") for n in HOST if n not in ("smh_pcg_jacobi_solve", "smh_cg_solve_many_host")})

# the 3 x 3 SPD tridiagonal system and its right-hand side
A3 = (np.array([0, 2, 5, 7], np.uint32), np.array([0, 1, 0, 1, 2, 1, 2], np.uint32), np.array([4, -1, -1, 4, -1, -1, 4], F64))
B3 = np.array([1.0, 2.0, 3.0])
X3 = np.linalg.solve(np.array([[4.0, -1, 0], [-1, 4, -1], [0, -1, 4]]), B3)


def square(n, dtype=F32):
    """n x n, tridiagonal (n = 3: A3), rows ascending, every diagonal stored"""
    if n == 3:
        return sm.SparseMatCRS.from_raw_parts(3, 3, A3[0], A3[1], A3[2].astype(dtype))
    assert n == 2
    return sm.SparseMatCRS.from_raw_parts(2, 2, [0, 2, 4], [0, 1, 0, 1], np.array([4, -1, -1, 4], dtype))


def factor(a, name=None):
    """what `name` takes as its preconditioner's handles for a: ILU(0)'s factor, for FSAI's entry points the pair (g, gt)"""
    if name in FSAI:
        g, gt, not_spd = a.fsai()
        assert not_spd is None
        return g, gt
    f, zero_pivot = a.ilu0()
    assert zero_pivot is None
    return f


def rect(dtype=F32):
    """2 x 3"""
    return sm.SparseMatCRS.from_raw_parts(2, 3, [0, 2, 4], [0, 1, 1, 2], np.array([4, -1, 4, -1], dtype))


def orphaned(dtype=F32):
    """2 x 2 with an orphaned entry (the first push of a replay into a SparseMatCRS), as test_trisolve_gpu.py builds it"""
    m = sm.SparseMatCRS.from_triplets([1, 0, 1, 0], [1, 0, 0, 1], np.ones(4, dtype), into_crs=True)
    assert m.orphans() == 1 and m.n_rows() == m.n_cols() == 2
    return m


class Out:
    """the out-parameters of a call, preset to 9: a refusal leaves them alone"""

    def __init__(self):
        self.iters, self.rr, self.brk, self.cycles = (C.c_size_t * 2)(9, 9), (C.c_double * 2)(9.0, 9.0), C.c_int(9), C.c_size_t(9)

    def untouched(self):
        return list(self.iters) == [9, 9] and list(self.rr) == [9.0, 9.0] and self.brk.value == 9 and self.cycles.value == 9


def handle_of(obj):
    return None if obj is None else obj._h


def entry(name):
    """the function a row calls and its signature"""
    fn = name.split(":")[0]
    return fn, SIG[fn[:-4] if fn.endswith("_vec") else fn]


def handles_after_matrix(name, f):
    """f: what the caller holds as the preconditioner's handle(s) -- passed where the entry point takes one (a "name:kind" row but
    for ILU's passes NULL), twice where it takes a pair and f is no pair"""
    takes = entry(name)[1][0]
    if takes == "f":
        return [handle_of(f)]
    if takes == "precond":
        kind = name.split(":")[1]
        return [_lib.PRECONDS[None if kind == "none" else kind], handle_of(f) if kind == "ilu" else None]
    if takes == "pair":
        g, gt = f if isinstance(f, tuple) else (f, f)
        return [handle_of(g), handle_of(gt)]
    return []


def tail(name, out, restart, middle):
    """what follows iter_max: restart where the entry point takes one, `middle` (the variant; the vec form's check_every), the outputs"""
    _, (_, takes_restart, outs) = entry(name)
    return ([restart] if takes_restart else []) + middle + [out.iters, out.rr] + [C.byref(getattr(out, o)) for o in outs]


def call_vec(name, m, b, x, out, f=None, check_every=0, restart=0, handles=None):
    """b, x: DenseVec (MultiVec for smh_cg_solve_many), or None.  handles: what follows the matrix, where handles_after_matrix's
    choice is not what the test wants"""
    L = sm.lib()
    if name == "smh_cg_solve_many":
        return L.smh_cg_solve_many(handle_of(m), handle_of(b), handle_of(x), TOL, ITER_MAX, check_every, out.iters, out.rr)
    args = [handle_of(m)] + (handles_after_matrix(name, f) if handles is None else handles) + [handle_of(b), handle_of(x), TOL, ITER_MAX]
    return getattr(L, entry(name)[0])(*(args + tail(name, out, restart, [_lib.VARIANTS["auto"], check_every])))


def call_host(name, m, b_ptr, b_len, x_ptr, x_len, out, f=None, restart=0, handles=None):
    """b_ptr, x_ptr: addresses or None.  smh_cg_solve_many_host takes one length and k = 1: x_len is not passed"""
    L = sm.lib()
    if name == "smh_cg_solve_many_host":
        return L.smh_cg_solve_many_host(handle_of(m), b_ptr, b_len, 1, x_ptr, TOL, ITER_MAX, out.iters, out.rr)
    args = [handle_of(m)] + (handles_after_matrix(name, f) if handles is None else handles) + [b_ptr, b_len, x_ptr, x_len, TOL, ITER_MAX]
    return getattr(L, entry(name)[0])(*(args + tail(name, out, restart, [_lib.VARIANTS["auto"]])))


def vec(name, values):
    values = np.ascontiguousarray(values)
    return sm.MultiVec.from_vecs(values[None, :]) if name == "smh_cg_solve_many" else sm.DenseVec.from_vec(values)


def values_of(name, v):
    return v.to_numpy()[0] if name == "smh_cg_solve_many" else v.to_numpy()


def refused(rc, want, what):
    status, text = want
    msg = sm.lib().smh_last_error().decode()
    assert rc == status and text in msg, (what, rc, msg, want)


# ---- the vec form -------------------------------------------------------------------------------------------------------------------
def dtype_text(name):
    return {"smh_cg_solve_vec": "dtype mismatch", "smh_cg_solve_many": "multi-vector dtype differs from the matrix's"}.get(name, VEC_DTYPE)


@pytest.mark.parametrize("name", VEC)
def test_vec_form_refusals(gpu, name):
    a = square(3)
    f = factor(a, name)
    sentinel = np.full(3, 7.0, F32)
    b, x = vec(name, np.ones(3, F32)), vec(name, sentinel)
    out = Out()

    def expect(rc, want, what):
        refused(rc, want, (name, what))
        assert np.array_equal(values_of(name, x), sentinel) and out.untouched(), (name, what)   # nothing was launched

    expect(call_vec(name, None, b, x, out, f), (INVALID, NULL_HANDLE), "NULL matrix")
    expect(call_vec(name, a, None, x, out, f), (INVALID, NULL_HANDLE), "NULL b")
    expect(call_vec(name, a, b, None, out, f), (INVALID, NULL_HANDLE), "NULL x")
    if name in ILU + FSAI:
        expect(call_vec(name, a, b, x, out, None), (INVALID, NULL_HANDLE), "NULL factor")
    expect(call_vec(name, a, vec(name, np.ones(4, F32)), x, out, f), (DIM, SIZE), "b of 4")
    expect(call_vec(name, a, vec(name, np.ones(3, F64)), x, out, f), (INVALID, dtype_text(name)), "b of the other dtype")
    x64 = vec(name, np.full(3, 7.0, F64))
    refused(call_vec(name, a, b, x64, out, f), (INVALID, dtype_text(name)), (name, "x of the other dtype"))
    assert np.array_equal(values_of(name, x64), np.full(3, 7.0)) and out.untouched()
    xs = vec(name, np.full(2, 7.0, F32))
    refused(call_vec(name, a, b, xs, out, f), (DIM, SIZE), (name, "x of 2"))
    assert np.array_equal(values_of(name, xs), np.full(2, 7.0, F32)) and out.untouched()
    # 2 x 3 with vectors of 2 (the rows) and of 3 (the columns)
    r = rect()
    x2, b2 = vec(name, sentinel[:2]), vec(name, np.ones(2, F32))
    for bb, xx in ((b2, x2), (b, x)):
        refused(call_vec(name, r, bb, xx, out, square(2)), (NOT_SQUARE, SYMMETRIC), (name, "2 x 3"))
        assert np.array_equal(values_of(name, xx)[:2], sentinel[:2]) and out.untouched()
    if name == "smh_cg_solve_many":   # ... and its own: the column counts, the output arrays
        expect(call_vec(name, a, sm.MultiVec.from_vecs(np.ones((2, 3), F32)), x, out), (DIM, SIZE), "k differs")
        L = sm.lib()
        expect(L.smh_cg_solve_many(a._h, b._h, x._h, TOL, ITER_MAX, 0, None, out.rr), (INVALID, "NULL output array"), "NULL iters")
        expect(L.smh_cg_solve_many(a._h, b._h, x._h, TOL, ITER_MAX, 0, out.iters, None), (INVALID, "NULL output array"), "NULL rr")
        expect(L.smh_cg_solve_many(a._h, b._h, x._h, TOL, ITER_MAX, 0, None, None), (INVALID, "NULL output array"), "NULL outputs")
    # where more than one check fires, the first one reported.  Wrong dtype, b is x, 2 x 3, wrong length: the dtype
    w = vec(name, np.full(4, 7.0, F64))
    refused(call_vec(name, r, w, w, out, square(2)), (INVALID, dtype_text(name)), (name, "all four"))
    # b is x, 2 x 3, wrong length: the same storage, but for smh_cg_solve_vec, which has no such check
    w = vec(name, np.full(4, 7.0, F32))
    want = (NOT_SQUARE, SYMMETRIC) if name == "smh_cg_solve_vec" else (INVALID, SAME)
    refused(call_vec(name, r, w, w, out, square(2)), want, (name, "b is x, 2 x 3, wrong length"))
    # 2 x 3 and a wrong length: not square
    refused(call_vec(name, r, vec(name, np.ones(4, F32)), w, out, square(2)), (NOT_SQUARE, SYMMETRIC), (name, "2 x 3, wrong length"))
    assert np.array_equal(values_of(name, w), np.full(4, 7.0, F32)) and out.untouched()
    # the call that all of these refused goes through
    assert call_vec(name, a, b, x, out, f) == OK and 0 < out.iters[0] <= ITER_MAX and out.iters[1] == 9


@pytest.mark.parametrize("name", VEC)
def test_vec_form_b_and_x_in_one_storage(gpu, name):
    """One handle for both, and two handles on one device array.  smh_cg_solve_vec does not refuse: it solves (r = b - A x is
    formed before x is first written, and b is not read again)."""
    a = square(3)
    f = factor(a, name)
    out = Out()
    if name == "smh_cg_solve_many":
        x = vec(name, B3.astype(F32))
        refused(call_vec(name, a, x, x, out), (INVALID, SAME), (name, "b is x"))
        assert np.array_equal(values_of(name, x), B3.astype(F32)) and out.untouched()
        return   # (a MultiVec owns its storage: no second handle on it)
    for second_handle in (False, True):
        x = sm.DenseVec.from_vec(B3.astype(F32))
        b = sm.DenseVec.from_device_ptr(x.data_ptr(), 3, F32, keep=x) if second_handle else x
        out = Out()
        rc = call_vec(name, a, b, x, out, f)
        if name == "smh_cg_solve_vec":
            assert rc == OK and 0 < out.iters[0] < ITER_MAX and np.sqrt(out.rr[0]) < TOL, (rc, list(out.iters), list(out.rr))
            assert np.allclose(x.to_numpy(), X3, rtol=0, atol=1e-5)
        else:
            refused(rc, (INVALID, SAME), (name, "one storage", second_handle))
            assert np.array_equal(x.to_numpy(), B3.astype(F32)) and out.untouched()


# ---- the host form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HOST)
def test_host_form_refusals(gpu, name):
    a = square(3)
    f = factor(a, name)
    sentinel = np.full(4, 7.0, F32)
    x, b = sentinel.copy(), np.ones(4, F32)
    out = Out()
    many = name == "smh_cg_solve_many_host"

    def expect(rc, want, what):
        refused(rc, want, (name, what))
        assert np.array_equal(x, sentinel) and out.untouched(), (name, what)   # nothing was launched, nothing copied back

    bp, xp = b.ctypes.data, x.ctypes.data
    expect(call_host(name, None, bp, 3, xp, 3, out, f), (INVALID, NULL_HANDLE), "NULL matrix")
    if name in ILU + FSAI:
        expect(call_host(name, a, bp, 3, xp, 3, out, None), (INVALID, NULL_HANDLE), "NULL factor")
    expect(call_host(name, a, bp, 4, xp, 4 if many else 3, out, f), (DIM, SIZE), "b of 4")
    if not many:
        expect(call_host(name, a, bp, 3, xp, 2, out, f), (DIM, SIZE), "x of 2")
    for n in (2, 3):   # 2 x 3 with vectors of 2 (the rows) and of 3 (the columns)
        expect(call_host(name, rect(), bp, n, xp, n, out, square(2)), (NOT_SQUARE, SYMMETRIC), "2 x 3")
    # a NULL host pointer with n > 0 (smh_cg_solve has no check of its own: the upload of the vector refuses)
    null_text = "NULL argument" if name == "smh_cg_solve" else "NULL host vector"
    expect(call_host(name, a, None, 3, xp, 3, out, f), (INVALID, null_text), "NULL b")
    expect(call_host(name, a, bp, 3, None, 3, out, f), (INVALID, null_text), "NULL x")
    expect(call_host(name, a, None, 3, None, 3, out, f), (INVALID, null_text), "NULL b and x")   # (before "the same storage")
    # where more than one check fires: not square, then the lengths, then the pointers
    expect(call_host(name, rect(), None, 4, None, 4, out, square(2)), (NOT_SQUARE, SYMMETRIC), "2 x 3, wrong length, NULL")
    expect(call_host(name, a, None, 4, None, 4, out, f), (DIM, SIZE), "wrong length, NULL")
    if many:
        L, r = sm.lib(), rect()
        expect(L.smh_cg_solve_many_host(None, bp, 3, 1, xp, TOL, ITER_MAX, None, out.rr), (INVALID, NULL_HANDLE), "NULL matrix, NULL iters")
        expect(L.smh_cg_solve_many_host(r._h, bp, 4, 1, xp, TOL, ITER_MAX, None, out.rr), (INVALID, "NULL output array"), "NULL iters")
        expect(L.smh_cg_solve_many_host(a._h, bp, 3, 1, xp, TOL, ITER_MAX, out.iters, None), (INVALID, "NULL output array"), "NULL rr")
        expect(L.smh_cg_solve_many_host(a._h, bp, 3, 0, xp, TOL, ITER_MAX, out.iters, out.rr), (INVALID, ""), "k = 0")
    # the call that all of these refused goes through
    assert call_host(name, a, bp, 3, xp, 3, out, f) == OK and 0 < out.iters[0] <= ITER_MAX and out.iters[1] == 9
    assert x[3] == 7.0 and not np.array_equal(x[:3], sentinel[:3])


@pytest.mark.parametrize("name", HOST)
def test_host_form_b_and_x_in_one_array(gpu, name):
    """Only BiCGSTAB's and GMRES's refuse; the others stage b and x apart and solve."""
    a = square(3)
    f = factor(a, name)
    x = B3.astype(F32)
    out = Out()
    rc = call_host(name, a, x.ctypes.data, 3, x.ctypes.data, 3, out, f)
    if name in HOST_REFUSES_SAME:
        refused(rc, (INVALID, SAME), name)
        assert np.array_equal(x, B3.astype(F32)) and out.untouched()
    else:
        assert rc == OK and 0 < out.iters[0] < ITER_MAX and np.sqrt(out.rr[0]) < TOL, (name, rc, list(out.iters), list(out.rr))
        assert np.allclose(x, X3, rtol=0, atol=1e-5)


# ---- the preconditioner's handle ----------------------------------------------------------------------------------------------------
def ilu_call(name, a, f, n, out):
    """vectors of n on a and f"""
    if name in VEC:
        return call_vec(name, a, sm.DenseVec.from_vec(np.ones(n, a.dtype)), sm.DenseVec.zeros(n, a.dtype), out, f)
    b, x = np.ones(n, a.dtype), np.zeros(n, a.dtype)
    rc = call_host(name, a, b.ctypes.data, n, x.ctypes.data, n, out, f)
    assert rc == OK or not x.any()
    return rc


def in_each_place(name, a, f):
    """f as the factor; for FSAI's pair f as g beside a gt that fits a, then as gt beside such a g (a 2 x 3 matrix is refused
    before either is looked at)"""
    if name not in FSAI:
        return [f]
    fits = square(a.n_rows(), a.dtype)
    return [(f, fits), (fits, f)]


@pytest.mark.parametrize("name", ILU + FSAI)
def test_ilu_pair_refusals(gpu, name):
    """What the matrix and the factor must agree in, in the order of the checks; FSAI's g against the matrix, then its gt, under
    FSAI's name.  (The fifth, a factor on another device, takes a second GPU to build: it is checked where there is one.)"""
    out = Out()
    a3 = square(3)
    who = "FSAI preconditioner" if name in FSAI else "ILU preconditioner"
    cases = [("the matrix is 2 x 3", rect(), square(2), 2, (NOT_SQUARE, SYMMETRIC)),
             ("the matrix is 2 x 3, and so is the factor", rect(), rect(), 2, (NOT_SQUARE, SYMMETRIC)),
             ("the factor is 2 x 3", square(2), rect(), 2, (NOT_SQUARE, who + ": the factor is not square")),
             ("the factor is 2 x 3 and of the other dtype", square(2), rect(F64), 2, (NOT_SQUARE, who + ": the factor is not square")),
             ("the factor is 2 x 2", a3, square(2), 3, (DIM, who + ": the factor's dimension differs from the matrix's")),
             ("the factor is 2 x 2 and of the other dtype", a3, square(2, F64), 3, (DIM, who + ": the factor's dimension differs from the matrix's")),
             ("the factor is of the other dtype", a3, square(3, F64), 3, (INVALID, who + ": the factor's dtype differs from the matrix's"))]
    for what, a, f, n, want in cases:
        for ff in in_each_place(name, a, f):
            refused(ilu_call(name, a, ff, n, out), want, (name, what))
            assert out.untouched(), (name, what)
    if name in FSAI:   # g is checked before gt
        refused(ilu_call(name, a3, (square(2), square(3, F64)), 3, out), (DIM, who + ": the factor's dimension differs from the matrix's"), (name, "g, then gt"))
        refused(ilu_call(name, a3, (square(3, F64), square(2)), 3, out), (INVALID, who + ": the factor's dtype differs from the matrix's"), (name, "g, then gt"))
    # the pair is checked before the vectors' lengths, after their dtype and storage (vec form)
    # -- but for FSAI's gt, which is checked after everything else the entry point checks of its arguments
    for place, ff in enumerate(in_each_place(name, a3, square(2))):
        want = (DIM, SIZE) if place == 1 else (DIM, who + ": the factor's dimension differs from the matrix's")
        refused(ilu_call(name, a3, ff, 2, out), want, (name, "pair, then lengths", place))
    if name in VEC:
        w = sm.DenseVec.zeros(3, F64)
        refused(call_vec(name, a3, w, w, out, square(2)), (INVALID, VEC_DTYPE), (name, "dtype, then pair"))
        w = sm.DenseVec.zeros(3, F32)
        refused(call_vec(name, a3, w, w, out, square(2)), (INVALID, SAME), (name, "storage, then pair"))
    assert out.untouched()
    print("%s: %d device(s)" % (name, gpu))
    if gpu >= 2:   # a factor on another device
        L = sm.lib()
        assert L.smh_set_device(1) == 0
        try:
            far = square(3)
        finally:
            assert L.smh_set_device(0) == 0
        for ff in in_each_place(name, a3, far):
            refused(ilu_call(name, a3, ff, 3, out), (INVALID, who + ": the factor and the matrix live on different devices"), (name, "devices"))
            assert out.untouched()


@pytest.mark.parametrize("name", TRI)
def test_orphaned_entry_in_the_preconditioner_handle(gpu, name):
    """SGS solves on the matrix itself, ILU on the factor, FSAI multiplies by either handle of its pair: an orphaned entry there is
    refused after the argument checks."""
    out = Out()
    who = "FSAI preconditioner" if name in FSAI else "ILU preconditioner" if name in ILU else "SGS preconditioner"
    m = orphaned()
    a = square(2) if name in ILU + FSAI else m
    sentinel = np.full(2, 7.0, F32)
    for f in in_each_place(name, a, m):
        if name in VEC:
            x = sm.DenseVec.from_vec(sentinel)
            rc = call_vec(name, a, sm.DenseVec.from_vec(np.ones(2, F32)), x, out, f)
            got = x.to_numpy()
        else:
            b, got = np.ones(2, F32), sentinel.copy()
            rc = call_host(name, a, b.ctypes.data, 2, got.ctypes.data, 2, out, f)
        refused(rc, (INVALID, who + ": the handle holds an orphaned entry"), name)
        assert np.array_equal(got, sentinel) and out.untouched()
        # ... after them: a wrong length is reported first
        if name in VEC:
            rc = call_vec(name, a, sm.DenseVec.from_vec(np.ones(3, F32)), sm.DenseVec.zeros(2, F32), out, f)
        else:
            rc = call_host(name, a, b.ctypes.data, 3, got.ctypes.data, 2, out, f)
        refused(rc, (DIM, SIZE), (name, "length first"))
        if name in GMRES:   # ... and so is a restart out of range
            if name in VEC:
                rc = call_vec(name, a, sm.DenseVec.from_vec(np.ones(2, F32)), sm.DenseVec.zeros(2, F32), out, f, restart=129)
            else:
                rc = call_host(name, a, b.ctypes.data, 2, got.ctypes.data, 2, out, f, restart=129)
            refused(rc, (INVALID, RESTART), (name, "restart first"))
        assert out.untouched()


# ---- what the preconditioned entry points and GMRES's have of their own -----------------------------------------------------------
def call3(name, a, out, f=None, n=3, **more):
    """name on a with b and x of n, through whichever form it is; x must come back as it went"""
    if name in VEC:
        x = sm.DenseVec.from_vec(np.full(n, 7.0, F32))
        rc = call_vec(name, a, sm.DenseVec.from_vec(np.ones(n, F32)), x, out, f, **more)
        got = x.to_numpy()
    else:
        b, got = np.ones(n, F32), np.full(n, 7.0, F32)
        rc = call_host(name, a, b.ctypes.data, n, got.ctypes.data, n, out, f, **more)
    assert np.array_equal(got, np.full(n, 7.0, F32)) and out.untouched(), name
    return rc


@pytest.mark.parametrize("name", rows(PRECOND, "_vec", ("ilu",)) + rows(PRECOND, "", ("ilu",)))
def test_precond_and_factor_come_first(gpu, name):
    """`precond` out of range, a factor beside a kind that takes none and ILU without one are refused before anything else -- a NULL
    matrix too."""
    out = Out()
    a = square(3)
    f = factor(a)
    J, S, I, N = (_lib.PRECONDS[k] for k in ("jacobi", "sgs", "ilu", None))
    for m in (a, None):
        for code in (-1, 4, 99):
            refused(call3(name, m, out, handles=[code, f._h]), (INVALID, "precond is %d: it must be one of SMH_PRECOND_*" % code), (name, code))
            refused(call3(name, m, out, handles=[code, None]), (INVALID, "precond is %d: it must be one of SMH_PRECOND_*" % code), (name, code))
        for code in (N, J, S):
            refused(call3(name, m, out, handles=[code, f._h]), (INVALID, "a factor handle goes with SMH_PRECOND_ILU alone"), (name, code))
        refused(call3(name, m, out, handles=[I, None]), (INVALID, NULL_HANDLE), (name, "ILU, NULL factor"))
    # ... before a wrong length and a restart out of range as well
    refused(call3(name, a, out, handles=[J, f._h], n=4, restart=129), (INVALID, "a factor handle goes with SMH_PRECOND_ILU alone"), (name, "first of three"))
    # ILU with a NULL factor says what a NULL matrix says; with both, so does the rest of the pair's checks
    refused(call3(name, rect(), out, handles=[I, None], n=2), (INVALID, NULL_HANDLE), (name, "ILU, NULL factor, 2 x 3"))


@pytest.mark.parametrize("name", FSAI)
def test_fsai_takes_both_handles(gpu, name):
    """a NULL g or gt is refused as a NULL matrix is, before anything else"""
    out = Out()
    a = square(3)
    g, gt = factor(a, name)
    for m in (a, None, rect()):
        for pair in ((None, gt), (g, None), (None, None)):
            refused(call3(name, m, out, pair, n=4, restart=129), (INVALID, NULL_HANDLE), (name, "NULL in the pair"))


@pytest.mark.parametrize("name", GMRES)
def test_restart_is_checked_last(gpu, name):
    """restart above 128 is refused, after every other argument check; 128 is taken, and 0 stands for 30"""
    out = Out()
    a = square(3)
    f = factor(a, name)
    for restart in (129, 1 << 40):
        refused(call3(name, a, out, f, restart=restart), (INVALID, "restart is %d: it must be at most 128 (0: the default, 30)" % restart), (name, restart))
    refused(call3(name, a, out, f, n=4, restart=129), (DIM, SIZE), (name, "lengths, then restart"))
    refused(call3(name, rect(), out, square(2), n=2, restart=129), (NOT_SQUARE, SYMMETRIC), (name, "square, then restart"))
    if name in ILU + FSAI:
        refused(call3(name, a, out, square(2), restart=129), (DIM, "preconditioner: the factor's dimension differs from the matrix's"), (name, "pair, then restart"))
    if name in VEC:
        w = sm.DenseVec.from_vec(np.full(3, 7.0, F32))
        refused(call_vec(name, a, w, w, out, f, restart=129), (INVALID, SAME), (name, "storage, then restart"))
    else:
        w = np.full(3, 7.0, F32)
        refused(call_host(name, a, w.ctypes.data, 3, w.ctypes.data, 3, out, f, restart=129), (INVALID, SAME), (name, "storage, then restart"))
        refused(call_host(name, a, None, 3, w.ctypes.data, 3, out, f, restart=129), (INVALID, "NULL host vector"), (name, "NULL b, then restart"))
    assert out.untouched()
    for restart in (128, 0, 1):
        out = Out()
        if name in VEC:
            x = sm.DenseVec.zeros(3, F32)
            rc = call_vec(name, a, sm.DenseVec.from_vec(B3.astype(F32)), x, out, f, restart=restart)
            xs = x.to_numpy()
        else:
            b, xs = B3.astype(F32), np.zeros(3, F32)
            rc = call_host(name, a, b.ctypes.data, 3, xs.ctypes.data, 3, out, f, restart=restart)
        print("%s restart %d: %d bodies, %d cycles, breakdown %d" % (name, restart, out.iters[0], out.cycles.value, out.brk.value))
        assert rc == OK and 0 < out.iters[0] <= ITER_MAX and out.cycles.value >= 1, (name, restart, rc)
        assert np.allclose(xs, X3, rtol=0, atol=1e-4)


# ---- check_every = 0 ----------------------------------------------------------------------------------------------------------------
def solve3(name, dtype, check_every):
    """(iterations, rr, x, breakdown) of the 3 x 3 system from x = 0, tol 1e-5, iter_max 20"""
    a = square(3, dtype)
    f = factor(a, name) if name in ILU + FSAI else None
    out = Out()
    if name in VEC:
        x = vec(name, np.zeros(3, dtype))
        assert call_vec(name, a, vec(name, B3.astype(dtype)), x, out, f, check_every) == OK, sm.lib().smh_last_error()
        xs = values_of(name, x)
    else:
        b, xs = B3.astype(dtype), np.zeros(3, dtype)
        assert call_host(name, a, b.ctypes.data, 3, xs.ctypes.data, 3, out, f) == OK, sm.lib().smh_last_error()
    assert out.iters[1] == 9 and out.rr[1] == 9.0
    return out.iters[0], out.rr[0], xs, out.brk.value


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", VEC + HOST)
def test_check_every_zero_is_the_default(gpu, name, dtype):
    """check_every = 0 (the host forms pass it themselves) gives what the explicit default gives -- 4 bodies per poll for CG and the
    k-column CG, 8 for the others -- and the solve converges: a stop test ends it before iter_max, sqrt(r.r) < tol."""
    it0, rr0, x0, brk0 = solve3(name, dtype, 0)
    print("%s %s: %d bodies, r.r = %g, breakdown %d" % (name, np.dtype(dtype).name, it0, rr0, brk0))
    # (GMRES's code 1 is a converged end too: by its third body the Krylov space of a 3 x 3 system is exhausted, and x is updated from it)
    assert 0 < it0 < ITER_MAX and np.sqrt(rr0) < TOL and brk0 in ((0, 1) if name in GMRES else (0, 9)), (it0, rr0, brk0)
    assert np.allclose(x0, X3, rtol=0, atol=1e-5)
    explicit = name if name in VEC else VEC_OF.get(name)
    if explicit is None:
        return   # (smh_pcg_jacobi_solve: no check_every anywhere; its batches are of 8)
    it1, rr1, x1, brk1 = solve3(explicit, dtype, DEFAULT_CHECK_EVERY[explicit])
    assert it0 == it1 and rr0 == rr1 and np.array_equal(x0, x1) and brk0 == brk1, (it0, it1, rr0, rr1, x0, x1)
