"""The device-resident thick-restart Lanczos eigensolver (eigsh.hip) pinned BIT FOR BIT to tests/eigsh_model.py's "device" mode:
the eigenvalues, the eigenvectors, the estimates, n_conv, restarts, products and the breakdown code -- f32 and f64, through both
entry points (smh_eigsh on host arrays, smh_eigsh_vec on a DenseVec and a MultiVec), with and without vectors, at the sizes where
each path of the sweeps is first entered, at basis widths around the dots' column tile and the rotation's output tile, for both
ends of the spectrum, on every breakdown code, through the STREAM, SEQ and AUTO products and two kernel families of
tests/kernel_forms.py.  The cases live in tests/eigsh_cases.py; tests/test_eigsh_model.py shows without a GPU that each of them
moves a bit under every wrong variant of the arithmetic that can touch it.

The model (not this file) says what the arithmetic is; tests/test_eigsh_model.py pins the model without a GPU."""
import ctypes as C

import numpy as np
import pytest

import eigsh_cases as ec
import eigsh_model as em
import gmres_cases
import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
WHICH_NAME = {em.LARGEST: "LA", em.SMALLEST: "SA"}
DP = C.POINTER(C.c_double)


def same(a, b):
    """bit equality (any NaN equals any NaN: its sign and payload are not arithmetic)"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def matrix(off, col, val):
    n = len(off) - 1
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)


class Got:
    def __init__(self, values, vectors, estimates, n_conv, restarts, products, breakdown):
        self.values, self.vectors, self.estimates = values, vectors, estimates
        self.n_conv, self.restarts, self.products, self.breakdown = n_conv, restarts, products, breakdown


SENTINEL = 7.0


def solve_host(a, start, k, ncv, which, tol, restart_max, variant="seq", vectors=True):
    """smh_eigsh: numpy arrays.  The outputs start as SENTINEL, so what a call does not write shows."""
    n = a.n_rows()
    start = np.ascontiguousarray(start, a.dtype)
    values, est = np.full(k, SENTINEL), np.full(k, SENTINEL)
    vecs = np.full((k, n), SENTINEL, a.dtype) if vectors else None
    n_conv, restarts, products, brk = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int()
    _lib.check(sm.lib().smh_eigsh(a._h, start.ctypes.data, n, k, ncv, which, tol, restart_max, _lib.VARIANTS[variant], values.ctypes.data_as(DP),
                                  vecs.ctypes.data if vectors else None, est.ctypes.data_as(DP), C.byref(n_conv), C.byref(restarts),
                                  C.byref(products), C.byref(brk)))
    if brk.value in (2, 3):  # nothing is returned: nothing was written
        assert (values == SENTINEL).all() and (est == SENTINEL).all() and (vecs is None or (vecs == SENTINEL).all())
        values = est = vecs = None
    return Got(values, vecs, est, n_conv.value, restarts.value, products.value, brk.value)


def solve_vec(a, start, k, ncv, which, tol, restart_max, variant="seq", vectors=True):
    """smh_eigsh_vec through SparseMatCRS.eigsh: a DenseVec start, a MultiVec of k columns"""
    sd = sm.DenseVec.from_vec(np.ascontiguousarray(start, a.dtype))
    r = a.eigsh(k, WHICH_NAME[which], ncv or None, tol if tol else 5e-324, restart_max, sd, vectors, variant)
    assert same(sd.to_numpy(), np.ascontiguousarray(start, a.dtype))  # (the start is read only)
    vecs = None
    if r.vectors is not None:
        assert r.vectors.count() == k and r.vectors.dim() == a.n_rows()
        vecs = r.vectors.to_numpy()
    return Got(r.values, vecs, r.estimates, r.n_conv, r.restarts, r.products, r.breakdown)


def assert_result(got, want, what, vectors=True):
    assert got.breakdown == want.breakdown, (what, "breakdown", got.breakdown, want.breakdown)
    assert got.products == want.products, (what, "products", got.products, want.products)
    assert got.restarts == want.restarts, (what, "restarts", got.restarts, want.restarts)
    assert got.n_conv == want.n_conv, (what, "n_conv", got.n_conv, want.n_conv)
    if want.values is None:
        assert got.values is None and got.vectors is None and got.estimates is None, what
        return
    assert same(got.values, want.values), (what, "values", got.values, want.values)
    assert same(got.estimates, want.estimates), (what, "estimates", got.estimates, want.estimates)
    if vectors:
        bad = np.argwhere(~((got.vectors == want.vectors) | (np.isnan(got.vectors) & np.isnan(want.vectors))))
        assert same(got.vectors, want.vectors), (what, "vectors", len(bad), bad[:5])
    else:
        assert got.vectors is None


def run_case(case, dtype, variant="seq", product=None, forms=("host", "vec")):
    """tol = 0 in a case means a pair converges on an exactly zero estimate alone: the vec form (whose Python surface reads 0 as the
    default) is handed the smallest positive double, under which no other estimate of these cases lies either -- asserted on the model."""
    off, col, val = case.matrix(dtype)
    start = case.start(dtype)
    want = em.eigsh(off, col, val, start, case.k, case.ncv, case.which, case.tol(dtype), case.restart_max, product=product)
    if case.tol(dtype) == 0.0 and want.estimates is not None and want.breakdown == 0:
        assert ((want.estimates == 0) | (want.estimates > 1e-300)).all()
    a = matrix(off, col, val)
    args = (a, start, case.k, case.ncv, case.which, case.tol(dtype), case.restart_max, variant)
    if "host" in forms:
        assert_result(solve_host(*args), want, (case.name, "host"))
    if "vec" in forms:
        assert_result(solve_vec(*args), want, (case.name, "vec"))
    return want, a, (off, col, val, start)


def ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ec.SIZES, ids=ids(ec.SIZES))
def test_bits_at_every_path_size(gpu, dtype, case):
    """n = 1, 2, 3 (m = n: one cycle, the whole space), 5; 253 .. 260 (every n mod V, one and two workgroups); 2049 / 2051 (nine
    workgroups).  k = 2, m = 6, tol = 0, two restarts; both entry points; LARGEST for odd n, SMALLEST for even."""
    want, _, _ = run_case(case, dtype)
    if case.n > 5:
        assert (want.restarts, want.products, want.breakdown, want.n_conv) == (2, 6 + 2 + 2, 0, 0)
    else:
        assert want.restarts == 0 and want.products <= case.n


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_past_the_grid_cap(gpu, dtype):
    """gmres_cases.big_n: the grid is at its cap of 512 workgroups and every thread makes a third trip over the 16-byte vectors.
    k = 1, m = 4, one restart (l = 2): six bodies."""
    n = gmres_cases.big_n(dtype)
    case = ec.Case("big", n, ec.tri, 1, 4, em.LARGEST, restart_max=1)
    want, _, _ = run_case(case, dtype)
    assert (want.restarts, want.products, want.breakdown) == (1, 6, 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ec.WIDTHS + [ec.WIDEST], ids=ids(ec.WIDTHS + [ec.WIDEST]))
def test_bits_at_basis_widths_around_the_tiles(gpu, dtype, case):
    """(k, m) on n = 130 with l = k + (m - k) // 2 and m on both sides of the dots' tile (8 columns) and of the rotation's output
    tile (8 columns): l = 2 (m = l + 1: a one-body cycle), 4, 5, 6, 8, 8, 9, 10, 17; k = 3, 4, 5: an smh_mvec with and without
    padding columns; m = 128 once (k = 30, l = 79: ten output tiles)."""
    want, _, _ = run_case(case, dtype)
    assert want.restarts == case.restart_max and want.breakdown == 0
    assert want.products == case.m() + case.restart_max * (case.m() - case.l())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ec.STOPS, ids=ids(ec.STOPS))
def test_bits_of_the_stops(gpu, dtype, case):
    """Converged inside the restart budget at both ends of the spectrum (n_conv == k); restart_max = 0 and 1 (n_conv < k, the k best
    pairs returned with their estimates); the default ncv.  With and without vectors."""
    want, a, (off, col, val, start) = run_case(case, dtype)
    if case.name.startswith("converges"):
        assert want.n_conv == case.k and 0 < want.restarts < case.restart_max
    else:
        assert want.n_conv < case.k and want.restarts == case.restart_max and np.isfinite(want.estimates).all()
    args = (a, start, case.k, case.ncv, case.which, case.tol(dtype), case.restart_max, "seq")
    assert_result(solve_host(*args, vectors=False), want, (case.name, "host, no vectors"), vectors=False)
    assert_result(solve_vec(*args, vectors=False), want, (case.name, "vec, no vectors"), vectors=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cases_and_breakdowns(gpu, dtype):
    """The exact cases of the CPU file against the model and against their literals."""
    literal = {"diag, start on three entries, k=2": (1, 3, 2), "diag, start on three entries, k=4": (1, 3, 3), "A = 2 I": (1, 1, 1),
               "zero start": (2, 0, 0), "infinite start": (2, 0, 0), "NaN in the matrix": (3, 6, 0)}
    for case in ec.EXACT:
        want, a, (off, col, val, start) = run_case(case, dtype)
        assert (want.breakdown, want.products, want.n_conv) == literal[case.name], case.name
        assert want.restarts == 0
    got = solve_host(matrix(*ec.two_i(5, dtype)), ec.e1(5), 1, 4, em.LARGEST, 1e-6, 10)
    assert got.values.tolist() == [2.0] and got.estimates.tolist() == [0.0] and got.vectors.tolist() == [[1.0, 0, 0, 0, 0]]
    case = ec.EXACT[1]  # k = 4 > 3 columns
    got = solve_host(matrix(*case.matrix(dtype)), case.start(dtype), 4, 7, em.SMALLEST, 1e-6, 10)
    assert np.isnan(got.values[3]) and np.isnan(got.estimates[3]) and (got.vectors[3] == 0).all() and got.estimates[:3].tolist() == [0.0] * 3
    assert np.abs(got.values[:3] - np.array([-2.0, 0.0, 2.0])).max() <= 4 * np.finfo(dtype).eps


def test_solves_are_reproducible(gpu):
    for n, dtype in ((257, np.float32), (2049, np.float64)):
        case = ec.Case("again", n, ec.tri, 3, 9, em.LARGEST, restart_max=3)
        off, col, val = case.matrix(dtype)
        a = matrix(off, col, val)
        args = (a, case.start(dtype), 3, 9, em.LARGEST, 0.0, 3)
        first = solve_vec(*args)
        for other in (solve_vec(*args), solve_host(*args), solve_host(*args)):
            assert (other.n_conv, other.restarts, other.products, other.breakdown) == (first.n_conv, first.restarts, first.products, first.breakdown)
            assert other.values.tobytes() == first.values.tobytes() and other.estimates.tobytes() == first.estimates.tobytes()
            assert other.vectors.tobytes() == first.vectors.tobytes()


# ---- the products ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stream_seq_and_auto_products(gpu, dtype):
    """The 12 x 12 grid operator, k = 3, m = 9, two restarts.  "seq" and "stream" are the oracle's product bit for bit (asserted for
    "stream"), so the model's default product; "auto": the model is fed the device's own checked product."""
    from test_solver_kernels_gpu import device_product
    off, col, val = em.grid_operator(12, 12, dtype, seed=3)
    case = ec.Case("grid 12 x 12", 144, lambda n, d: (off, col, val), 3, 9, em.SMALLEST)
    start = case.start(dtype)
    a = matrix(off, col, val)
    assert same(a.mvp(start, variant="stream"), oracle.spmv(off, col, val, start)), "K1s product not bit-exact"
    for variant in ("seq", "stream"):
        want, _, _ = run_case(case, dtype, variant)
        assert (want.restarts, want.products, want.breakdown) == (2, 9 + 3 + 3, 0)
    run_case(case, dtype, "auto", product=device_product(a, "auto", off, col, val))


FAMILIES = [("k1r-col16", np.float32), ("colblock", np.float64)]


@pytest.mark.parametrize("name,dtype", FAMILIES, ids=["%s-%s" % (n, np.dtype(d).name) for n, d in FAMILIES])
def test_equal_the_model_fed_by_the_checked_device_product(gpu, name, dtype):
    """Two further kernel families of tests/kernel_forms.py, each in the form it is named for.  Their matrices need not be symmetric:
    the recurrence is arithmetic all the same, and the model takes every product from the device's own eager product of the same
    variant on the same handle, checked before it is used.  k = 2, m = 6, one restart."""
    from kernel_forms import CONFIGS, env
    from test_solver_kernels_gpu import device_product
    cfg = CONFIGS[name]
    off, col, val = cfg.build(dtype)
    n = len(off) - 1
    start = em.start_vector(n, dtype, seed=5)
    a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    fused_env = dict(SMH_CG_FUSED_DOT=None, SMH_STREAM_RPT=None) if cfg.fused else {}
    with env(**cfg.env, **fused_env):
        cfg.knobs(a)
        a.prepare(cfg.variant)
        cfg.check(a)
        want = em.eigsh(off, col, val, start, 2, 6, em.LARGEST, 0.0, 1, product=device_product(a, cfg.variant, off, col, val))
        assert (want.restarts, want.products) == (1, 6 + 2) and want.breakdown in (0, 3)
        assert_result(solve_host(a, start, 2, 6, em.LARGEST, 0.0, 1, cfg.variant), want, (name, "host"))
        assert_result(solve_vec(a, start, 2, 6, em.LARGEST, 0.0, 1, cfg.variant), want, (name, "vec"))
        cfg.check(a)  # (the solves have changed no form)


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mvp_many_on_the_returned_vectors_reproduces_theta_x(gpu, dtype):
    """SparseMatCRS.eigsh with its defaults but k, ncv and tol on tridiag 100: n_conv == k, and A X from mvp_many on the returned
    MultiVec equals theta_c x_c within the CPU file's residual bound, 2 tol max|theta| per column (two-norm, f64)."""
    off, col, val = em.tridiag_sym(100, dtype, seed=0)
    a = matrix(off, col, val)
    tol = ec.conv_tol(dtype)
    r = a.eigsh(k=4, which="LA", ncv=20, tol=tol, variant="seq")
    assert r.n_conv == 4 and r.breakdown == 0 and isinstance(r.vectors, sm.MultiVec)
    ax = a.mvp_many(r.vectors).to_numpy().astype(np.float64)
    x = r.vectors.to_numpy().astype(np.float64)
    lam = np.linalg.eigvalsh(em.dense_of(off, col, val))
    want = em.eigsh(off, col, val, em.start_vector(100, dtype), 4, 20, em.LARGEST, tol, 1000)
    bound = 2 * tol * want.theta_max
    for c in range(4):
        res = float(np.linalg.norm(ax[c] - r.values[c] * x[c]))
        print(np.dtype(dtype).name, c, r.values[c], res, bound)
        assert res <= bound and abs(r.values[c] - lam[::-1][c]) <= bound
    assert same(r.values, want.values) and same(x.astype(dtype), want.vectors)  # (v0 = None is default_rng(0).standard_normal(n))


# ---- statuses --------------------------------------------------------------------------------------------------------------------
def test_statuses_leave_the_outputs_untouched(gpu):
    f = np.float64
    off, col, val = em.tridiag_sym(5, f)
    a = matrix(off, col, val)
    wide = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 2], np.ones(2, f))
    L = sm.lib()
    values, est, vecs = np.full(8, SENTINEL), np.full(8, SENTINEL), np.full((8, 5), SENTINEL)
    outs = [C.c_size_t(77), C.c_size_t(77), C.c_size_t(77), C.c_int(77)]
    start = np.ones(5, f)
    sd, sd4, s32 = sm.DenseVec.from_vec(start), sm.DenseVec.from_vec(np.ones(4, f)), sm.DenseVec.from_vec(np.ones(5, np.float32))
    mv2, mv3, mv2_32, mv2_n4 = sm.MultiVec.zeros(5, 2, f), sm.MultiVec.zeros(5, 3, f), sm.MultiVec.zeros(5, 2, np.float32), sm.MultiVec.zeros(4, 2, f)

    def host(m, sptr, slen, k, ncv, which):
        return L.smh_eigsh(m, sptr, slen, k, ncv, which, 1e-10, 10, _lib.VARIANTS["seq"], values.ctypes.data_as(DP), vecs.ctypes.data,
                           est.ctypes.data_as(DP), C.byref(outs[0]), C.byref(outs[1]), C.byref(outs[2]), C.byref(outs[3]))

    def vec(m, s, ev, k, ncv, which):
        return L.smh_eigsh_vec(m, s, ev, k, ncv, which, 1e-10, 10, _lib.VARIANTS["seq"], values.ctypes.data_as(DP), est.ctypes.data_as(DP),
                               C.byref(outs[0]), C.byref(outs[1]), C.byref(outs[2]), C.byref(outs[3]))

    sp = start.ctypes.data
    inv, dim, nsq = _lib.SMH_ERR_INVALID, _lib.SMH_ERR_DIM_MISMATCH, _lib.SMH_ERR_NOT_SQUARE
    assert host(None, sp, 5, 2, 0, 0) == inv and b"NULL handle" in L.smh_last_error()
    assert host(a._h, None, 5, 2, 0, 0) == inv
    assert host(wide._h, sp, 2, 1, 0, 0) == nsq and b"Matrix is not symmetric" in L.smh_last_error()
    assert host(a._h, sp, 4, 2, 0, 0) == dim and b"Matrix and vector size mismatch" in L.smh_last_error()
    assert host(a._h, sp, 5, 0, 0, 0) == inv and host(a._h, sp, 5, 6, 0, 0) == inv          # k == 0, k > n
    assert host(a._h, sp, 5, 2, 3, 0) == inv and b"ncv" in L.smh_last_error()                # ncv < k + 2
    assert host(a._h, sp, 5, 2, 0, 2) == inv and host(a._h, sp, 5, 2, 0, -1) == inv          # which
    assert vec(None, sd._h, mv2._h, 2, 0, 0) == inv and vec(a._h, None, mv2._h, 2, 0, 0) == inv
    assert vec(wide._h, sd._h, None, 1, 0, 0) == nsq
    assert vec(a._h, sd4._h, mv2._h, 2, 0, 0) == dim and vec(a._h, sd._h, mv2_n4._h, 2, 0, 0) == dim
    assert vec(a._h, s32._h, mv2._h, 2, 0, 0) == inv and vec(a._h, sd._h, mv2_32._h, 2, 0, 0) == inv   # a dtype that is not the matrix's
    assert vec(a._h, sd._h, mv3._h, 2, 0, 0) == inv and b"evecs" in L.smh_last_error()       # evecs->count() != k
    big = matrix(*em.tridiag_sym(200, f))
    s200 = np.ones(200, f)
    assert L.smh_eigsh(big._h, s200.ctypes.data, 200, 2, 129, 0, 1e-10, 10, 0, None, None, None, None, None, None, None) == inv   # ncv > 128
    assert L.smh_eigsh(big._h, s200.ctypes.data, 200, 127, 0, 0, 1e-10, 10, 0, None, None, None, None, None, None, None) == inv  # k + 2 > 128
    # nothing was written
    assert (values == SENTINEL).all() and (est == SENTINEL).all() and (vecs == SENTINEL).all() and [o.value for o in outs] == [77] * 4
    assert (mv2.to_numpy() == 0).all() and (mv3.to_numpy() == 0).all()
    # ... and every output pointer may be NULL; ncv is clipped to n (9 -> 5), k + 2 > n takes m = n
    v = _lib.VARIANTS["seq"]
    assert L.smh_eigsh(a._h, sp, 5, 2, 9, 0, 1e-10, 10, v, None, None, None, None, None, None, None) == 0
    assert L.smh_eigsh_vec(a._h, sd._h, None, 4, 0, 1, 1e-10, 10, v, None, None, None, None, None, None) == 0
    want = em.eigsh(off, col, val, start, 4, 0, em.SMALLEST, 1e-10, 10)
    assert_result(solve_host(a, start, 4, 0, em.SMALLEST, 1e-10, 10), want, "k + 2 > n")
    assert want.restarts == 0 and want.products == 5
