"""CPU: tests/eigsh_model.py -- the contract of the device-resident thick-restart Lanczos eigensolver (eigsh.hip) -- : the Jacobi
step on arrowhead + tridiagonal inputs, convergence with the true residual and the agreement with dense eigvalsh on every
convergence case, the cases worked by hand, the sensitivity of the GPU file's cases to every wrong variant of the arithmetic, and
the declarations and device-free refusals of the two entry points."""
import os
import re

import numpy as np
import pytest

import eigsh_cases as ec
import eigsh_model as em
import oracle
import sparsemat_amd as sm
from sparsemat_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
MODES = ["sequential", "device", "wide"]
EPS64 = float(np.finfo(np.float64).eps)


# ---- the Jacobi step ---------------------------------------------------------------------------------------------------------
def arrowhead(m, seed):
    """an arrowhead of l = m // 3 locked values coupled to row l, then a tridiagonal tail: entries of size one"""
    rng = np.random.default_rng(seed)
    l = m // 3
    return em.projected(rng.uniform(-2, 2, l), rng.uniform(-1, 1, l), rng.uniform(-2, 2, m), rng.uniform(0.1, 1, m), l, m)


# The worst c = max(|Y^T Y - I|_F, |B - Y diag(theta) Y^T|_F, max|theta - eigvalsh|) / (eps64 m |B|_F) the model shows on these
# cases is 1.24, at m = 18 in the reconstruction (printed by the test; |Y^T Y - I| reaches 0.87, theta against eigvalsh 0.35); the bound asserted is four times that.
JACOBI_WORST_C = 1.24
JACOBI_C = 4 * JACOBI_WORST_C


def test_jacobi_step_on_arrowhead_plus_tridiagonal_inputs():
    worst = 0.0
    for m in list(range(2, 41)) + [128]:
        b = arrowhead(m, m)
        theta, y, sweeps = em.jacobi(b)
        norm = float(np.linalg.norm(b))
        c = max(float(np.linalg.norm(y.T @ y - np.eye(m))), float(np.linalg.norm(b - (y * theta) @ y.T)),
                float(np.abs(theta - np.linalg.eigvalsh(b)).max())) / (EPS64 * m * norm)
        worst = max(worst, c)
        assert (np.diff(theta) >= 0).all() and sweeps < em.MAX_SWEEPS
        assert c <= JACOBI_C, (m, c)
    print("worst c", worst)
    assert worst >= JACOBI_WORST_C / 4  # (the recorded figure is the model's, not a guess)


def test_jacobi_corners():
    """a diagonal matrix: one sweep, no rotation; ties keep their index order; a tiny off-diagonal next to a huge diagonal is
    zeroed by the skip rule; a zero matrix; m = 1"""
    theta, y, sweeps = em.jacobi(np.diag([3.0, 1.0, 1.0, 2.0]))
    assert theta.tolist() == [1.0, 1.0, 2.0, 3.0] and sweeps == 1
    assert y.tolist() == [[0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
    theta, y, sweeps = em.jacobi(np.array([[1e300, 1e-300], [1e-300, -1e300]]))
    assert theta.tolist() == [-1e300, 1e300] and sweeps == 1
    theta, y, sweeps = em.jacobi(np.array([[0.0, 1.0], [1.0, 0.0]]))  # tau = 0: t = 1, a rotation by 45 degrees
    assert np.abs(theta - np.array([-1.0, 1.0])).max() <= 2 * EPS64 and sweeps == 2
    assert em.jacobi(np.zeros((3, 3)))[0].tolist() == [0, 0, 0] and em.jacobi(np.array([[5.0]]))[0].tolist() == [5.0]


# ---- convergence, the true residual, the agreement with eigvalsh ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name,build,n", ec.CONVERGENCE, ids=[c[0] for c in ec.CONVERGENCE])
def test_convergence_true_residual_and_agreement(name, build, n, dtype):
    """Every convergence case and dtype, LARGEST and SMALLEST, (k, m) = (1, 8), (4, 20), (8, 24), tol = 1e-10 in f64 and 1e-4 in
    f32, in "device" mode: n_conv == k; every returned pair has a true residual |A x - theta x| (two-norm, formed in f64 with the
    oracle's product) of at most 2 tol max|theta|; every theta_i lies within that bound of the i-th extreme eigenvalue of dense
    eigvalsh."""
    off, col, val = build(dtype)
    val64 = val.astype(np.float64)
    lam = np.linalg.eigvalsh(em.dense_of(off, col, val))
    assert np.diff(lam).min() > 0  # (no multiple eigenvalue)
    tol = ec.conv_tol(dtype)
    start = em.start_vector(n, dtype, seed=1)
    for which in (em.LARGEST, em.SMALLEST):
        extreme = lam[::-1] if which == em.LARGEST else lam
        for k, m in ec.KM:
            got = em.eigsh(off, col, val, start, k, m, which, tol, 400)
            assert got.n_conv == k and got.breakdown == 0, (name, which, k, m, got.n_conv, got.restarts)
            bound = 2 * tol * got.theta_max  # (max|theta| over the last cycle's m Ritz values: the stop test's own scale)
            worst_res = worst_err = 0.0
            for i in range(k):
                x = got.vectors[i].astype(np.float64)
                res = float(np.linalg.norm(oracle.spmv(off, col, val64, x) - got.values[i] * x))
                worst_res, worst_err = max(worst_res, res), max(worst_err, abs(got.values[i] - extreme[i]))
                assert res <= bound, (name, which, k, m, i, res, bound)
                assert abs(got.values[i] - extreme[i]) <= bound, (name, which, k, m, i, got.values[i], extreme[i])
            print(np.dtype(dtype).name, name, "LA" if which == em.LARGEST else "SA", k, m, "restarts", got.restarts, "products", got.products,
                  "residual / (tol max|theta|) %.3f" % (worst_res / (bound / 2)), "|theta - lambda| %.2e" % worst_err)


@pytest.mark.parametrize("mode", ["sequential", "wide"])
def test_other_reduction_modes_converge_too(mode):
    off, col, val = ec.CONVERGENCE[0][1](np.float64)
    lam = np.linalg.eigvalsh(em.dense_of(off, col, val))
    got = em.eigsh(off, col, val, em.start_vector(100, np.float64, seed=1), 4, 20, em.LARGEST, 1e-10, 400, mode=mode)
    assert got.n_conv == 4 and np.abs(got.values - lam[::-1][:4]).max() <= 2e-10 * np.abs(lam).max()


# ---- the cases worked by hand ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cases(dtype, mode):
    eps = float(np.finfo(dtype).eps)
    by_name = {c.name: c for c in ec.EXACT}
    # A = diag(-2, 7, 0, 9, 2, ..), the start (3, 2, 3) on entries 0, 2, 4: v_0 is symmetric about the middle entry and A v_0
    # antisymmetric, so alpha_0 = 0 exactly; the three eigenvalues after three bodies, the third w exactly zero: breakdown 1
    got = ec.run_model(by_name["diag, start on three entries, k=2"], dtype, mode=mode)
    assert (got.breakdown, got.products, got.restarts, got.n_conv) == (1, 3, 0, 2) and got.estimates.tolist() == [0.0, 0.0]
    assert np.abs(got.values - np.array([2.0, 0.0])).max() <= 4 * eps
    x = got.vectors.astype(np.float64)
    assert np.abs(np.abs(x[0]) - np.eye(8)[4]).max() <= 4 * eps and np.abs(np.abs(x[1]) - np.eye(8)[2]).max() <= 4 * eps
    got = ec.run_model(by_name["diag, start on three entries, k=4"], dtype, mode=mode)
    assert (got.breakdown, got.products, got.n_conv) == (1, 3, 3) and np.abs(got.values[:3] - np.array([-2.0, 0.0, 2.0])).max() <= 4 * eps
    assert np.isnan(got.values[3]) and np.isnan(got.estimates[3]) and (got.vectors[3] == 0).all()
    # A = 2 I, v = e_1: w = 2 e_1, h1_0 = 2, w = 0, h2_0 = 0, alpha_0 = 2, beta_0 = 0: breakdown 1 in the first body
    got = ec.run_model(by_name["A = 2 I"], dtype, mode=mode)
    assert (got.breakdown, got.products, got.restarts, got.n_conv) == (1, 1, 0, 1)
    assert got.values.tolist() == [2.0] and got.estimates.tolist() == [0.0] and got.vectors.tolist() == [[1.0, 0, 0, 0, 0]]
    # a zero start, a start that is not finite: breakdown 2, nothing returned, no product
    for name in ("zero start", "infinite start"):
        got = ec.run_model(by_name[name], dtype, mode=mode)
        assert (got.breakdown, got.products, got.n_conv) == (2, 0, 0) and got.values is None and got.vectors is None and got.estimates is None
    # a NaN in the matrix: the cycle runs its m bodies (NaN compares false), then breakdown 3, nothing returned
    got = ec.run_model(by_name["NaN in the matrix"], dtype, mode=mode)
    assert (got.breakdown, got.products, got.restarts, got.n_conv) == (3, 6, 0, 0) and got.values is None


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tiny_dimensions_take_the_whole_space(dtype):
    """n = 1, 2, 3 with m = n: one cycle of at most n bodies, no restart; the Ritz values are the eigenvalues to a few eps |A|"""
    eps = float(np.finfo(dtype).eps)
    for n in (1, 2, 3):
        off, col, val = ec.tri(n, dtype)
        lam = np.linalg.eigvalsh(em.dense_of(off, col, val))
        for which in (em.LARGEST, em.SMALLEST):
            for k in range(1, n + 1):
                assert em.clip_ncv(n, k, 0) == n and em.clip_ncv(n, k, 20) == n
                got = em.eigsh(off, col, val, em.start_vector(n, dtype, seed=n), k, 0, which, 1e-3, 5)
                assert got.restarts == 0 and got.products <= n and got.breakdown in (0, 1)
                want = (lam[::-1] if which == em.LARGEST else lam)[:k]
                assert np.abs(got.values - want).max() <= 16 * eps * np.abs(lam).max(), (n, k, got.values, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_an_exhausted_restart_budget_returns_the_best_pairs(dtype):
    by_name = {c.name: c for c in ec.STOPS}
    for name, restarts in (("restart_max 0", 0), ("restart_max 1", 1)):
        got = ec.run_model(by_name[name], dtype)
        assert got.restarts == restarts and got.n_conv < 4 and got.breakdown == 0
        assert np.isfinite(got.values).all() and (got.estimates[got.n_conv:] > 0).any() and got.vectors.shape == (4, 100)
        assert got.products == 20 + restarts * (20 - 12)


def test_clip_ncv():
    assert em.clip_ncv(100, 6, 0) == 20 and em.clip_ncv(100, 12, 0) == 25 and em.clip_ncv(15, 6, 0) == 15 and em.clip_ncv(1000, 100, 0) == 128 and em.clip_ncv(1000, 127, 0) is None
    assert em.clip_ncv(100, 6, 8) == 8 and em.clip_ncv(100, 6, 7) is None and em.clip_ncv(200, 6, 129) is None and em.clip_ncv(200, 6, 128) == 128 and em.clip_ncv(100, 6, 129) == 100
    assert em.clip_ncv(5, 4, 0) == 5 and em.clip_ncv(5, 5, 3) == 5 and em.clip_ncv(5, 0, 0) is None and em.clip_ncv(5, 6, 0) is None
    assert em.clip_ncv(7, 2, 200) == 7 and em.clip_ncv(200, 199, 0) is None


# ---- what the bit comparisons of the GPU file can tell apart ----------------------------------------------------------------------
def bits(r):
    if r.values is None:
        return None, r.n_conv, r.restarts, r.products, r.breakdown
    return r.values.tobytes(), r.vectors.tobytes(), r.estimates.tobytes(), r.n_conv, r.restarts, r.products, r.breakdown


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gpu_cases_move_under_every_wrong_variant(dtype):
    """Every case tests/test_eigsh_gpu.py compares bit for bit (eigsh_cases.BIT_CASES; the large size runs the same arithmetic)
    gives other bits under each wrong variant that can touch it.  What cannot tell: the exact cases and those that return nothing
    (case.exact); n <= 5 (sums of a handful of terms, one cycle); for "computed coupling" a case without a restart (no coupling
    exists); "rotation from zero" can move the sign of a zero alone (0 + p and p differ only for p = -0), which no
    case shows: it is asserted to give the same NUMBERS everywhere.
    Sequential sums in place of the device's tree move every case too."""
    for case in ec.BIT_CASES:
        want = ec.run_model(case, dtype)
        if case.exact or case.n <= 5:
            continue
        variants = em.WRONG[1:] + ("sequential",)
        if case is ec.WIDEST:  # (two cycles of 128 columns: the two variants that reach the rotation of 79 columns and the update)
            variants = ("rotation descending", "fma")
        for wrong in variants:
            other = ec.run_model(case, dtype, mode="sequential") if wrong == "sequential" else ec.run_model(case, dtype, wrong=wrong)
            if wrong == "rotation from zero":
                assert np.array_equal(other.vectors, want.vectors, equal_nan=True) and other.values.tobytes() == want.values.tobytes(), case.name
                continue
            blind = wrong == "computed coupling" and want.restarts == 0
            # the diagonal case is three bodies on three entries: sums of three terms have one order, and its single-column updates
            # of exact zeros cannot show an FMA or an order
            blind = blind or (case.name.startswith("diag") and wrong in ("fma", "descending", "sequential", "alpha pass 1", "one pass"))
            if not blind:
                assert bits(other) != bits(want), (case.name, wrong)


# ---- the product callable -----------------------------------------------------------------------------------------------------
def test_product_callable_is_what_the_model_consumes():
    off, col, val = em.tridiag_sym(100, np.float64, seed=0)
    start = em.start_vector(100, np.float64)
    calls = []

    def product(v):
        calls.append(v.copy())
        return oracle.spmv(off, col, val, v)
    want = em.eigsh(off, col, val, start, 2, 6, em.LARGEST, 0.0, 2)
    got = em.eigsh(off, col, val, start, 2, 6, em.LARGEST, 0.0, 2, product=product)
    assert bits(got) == bits(want) and len(calls) == got.products == 6 + 2 + 2


# ---- declarations and statuses ----------------------------------------------------------------------------------------------------
def test_binding_and_header_declare_both_entry_points():
    header = open(os.path.join(ROOT, "include", "sparsemat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("smh_eigsh", 16), ("smh_eigsh_vec", 15)):
        assert name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == n_args, (name, len(argtypes))
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert decl and len(decl.group(1).split(",")) == n_args, name
    assert re.search(r"#define\s+SMH_EIGSH_LARGEST\s+0\b", code) and re.search(r"#define\s+SMH_EIGSH_SMALLEST\s+1\b", code)
    assert (_lib.SMH_EIGSH_LARGEST, _lib.SMH_EIGSH_SMALLEST) == (0, 1) and _lib.EIGSH_WHICH == {"LA": 0, "SA": 1}
    assert re.search(r"#define\s+SMH_ABI_VERSION\s+3\b", code)
    # the statuses are decided before any device call: a NULL handle is refused where there is no device either
    L = sm.lib()
    assert L.smh_eigsh(None, None, 0, 1, 0, 0, 0.0, 1, 0, None, None, None, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert b"NULL handle" in L.smh_last_error()
    assert L.smh_eigsh_vec(None, None, None, 1, 0, 0, 0.0, 1, 0, None, None, None, None, None, None) == _lib.SMH_ERR_INVALID
    assert b"NULL handle" in L.smh_last_error()
    rust = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    assert "pub fn smh_eigsh(" in rust and "pub fn smh_eigsh_vec(" in rust
    hpp = open(os.path.join(ROOT, "include", "sparsemat.hpp")).read()
    assert re.search(r"\bclass\s+Lanczos\b", hpp)
