"""CG (cg.hip), Jacobi-PCG (pcg.hip) and BiCGSTAB (bicgstab.hip) pinned BIT FOR BIT through every product kernel family, each in
the form it is named for (asserted through the handle's own getters, before and after the solves): x, the number of entered
bodies, f64(r.r) and BiCGSTAB's breakdown code equal tests/cg_model.py / tests/bicgstab_model.py in "device" mode, the model
taking every product -- the initial residual's included -- from the DEVICE's eager product of the same variant on the same
handle (device_product), which is held to the suite's parity bound against the oracle (util.assert_spmv_close) before the
model may use it -- and, for the vector family and merge, to the oracle's CPU model of the kernel's own summation order
(oracle.spmv_lanes / oracle.spmv_merge, pinned in tests/test_spmv_order_model.py) bit for bit in every row.  So the model is never
anchored to the code under test alone, and no tolerance appears in this file.  The matrices and CONFIGS live in
tests/kernel_forms.py, shared with tests/test_spmv_order_gpu.py.

The statement per case: x0 random, tol = 0, iter_max = 11; check_every = 4 on the DenseVec entry points (three replays of the
captured batch, the last body a no-op) and the default on the host entry points (CG 4; PCG and BiCGSTAB 8: one replay and three
plain launches); each solve twice on the same handle (the second captures its graph anew).  For one value type per
configuration also a stop on tol in the middle of a batch (stop_tolerance).  The premise -- three eager products of one x and
one replayed from a graph captured on a side stream have the same bytes -- is asserted first on every matrix here.

The matrices (all square, symmetric in their non-zero values, strictly diagonally dominant with a positive diagonal: SPD;
off-diagonal values in (-1, 0), a_ii = 1 + sum_j |a_ij|):
  band(n, w, L)    row i holds the diagonal and 15 pairs i -+ d (the same 15 offsets d <= w in every row, 1 and w among them),
                   ascending; columns that fall off the matrix are replaced by stored 0.0 at unused columns next to the
                   diagonal, so every row has L = 31 entries, or 32 with one more stored zero (all 16-byte chunks row-aligned)
  scattered(n)     4 random pairs per row (about 9 entries with the diagonal), every 997th row and column about 3000 more
                   (hubs = False: none), rows stored in random order
  arrowhead(n)     40 hub rows and columns of about 2000 entries, 2 random pairs in every row (about 15 entries with the hub
                   columns), stored in random order
  stencil7(g)      the 7-point pattern of oracle.laplace3d(*g) with non-constant coefficients
  laplace3d(24^3)  the oracle's constant-coefficient Laplacian (two distinct values: K1s XD-V's dictionary)
The shapes are the smallest at which each form engages; what the getters must report is in CONFIGS.  The final numbers:
band(20 000, 4000, 31 | 32) for K1 and the single-window K1r forms; band(48 000, 10 000, 32) for the 32 768-column ring (at 30 000
rows the 16 384-column ring still serves 53 % of the rows and the plan keeps it); stencil7(130 x 130 x 6) for the banded ring (a
48 x 48 x 24 grid fits one window); scattered(40 000) for merge (316 tiles), K2c (5 blocks of 8192 columns) and K2t (3 slices),
without its hubs for K2f; arrowhead(8000) for K2s (40 long rows); 24^3 for K1s (the stage forced: x is under 1 MB).

Every case above prepares its handle first.  The last test sends a fresh handle of every configuration straight into a product and
holds it to the prepared one: same bytes, same forms, same resolution."""
import math

import numpy as np
import pytest
import torch

import bicgstab_model as bm
import cg_model
import oracle
import sparsemat_amd as sm
from kernel_forms import CONFIGS, F32, F64, config_matrix, env, same
from util import assert_spmv_close

pytestmark = pytest.mark.gpu

ITER_MAX = 11
CHECK_EVERY = 4


CASES = [pytest.param(name, dt, id="%s-%s" % (name, "f32" if dt == F32 else "f64")) for name, c in CONFIGS.items() for dt in c.dtypes]


# ---- the device's product, checked -------------------------------------------------------------------------------------------
def order_model(m, variant, off, col, val):
    """The CPU model of the device's own summation order for the lane-group kernels (oracle.spmv_lanes at the handle's lanes; the
    arrays are owned, hence padded: K1r has no tail) and the merge-path kernel (oracle.spmv_merge); None for the other families,
    which test_stream_gpu.py, test_colblock_gpu.py and test_tiled_gpu.py pin."""
    family, lanes = m.resolved_variant()
    if variant != "auto":
        family = variant
    if family == "vector":
        return lambda v: oracle.spmv_lanes(off, col, val, v, lanes)
    if family == "merge":
        assert m.merge_table()[2] == oracle.MERGE_TILE
        return lambda v: oracle.spmv_merge(off, col, val, v)
    return None


def device_product(m, variant, off, col, val):
    """product(v) = m.mvp(v, variant) computed eagerly on the device, handed on only after util.assert_spmv_close has held it to the
    parity bound against the oracle's product and -- vector family and merge -- after it has equalled the CPU model of the kernel's
    summation order in every row, bit for bit.  (A vector met before is answered from the first, checked, product: the stop cases
    walk the same iterates again.)"""
    seen = {}
    model = order_model(m, variant, off, col, val)

    def product(v):
        v = np.ascontiguousarray(v, val.dtype)
        key = v.tobytes()
        if key not in seen:
            y = m.mvp(v, variant=variant)
            assert_spmv_close(y, off, col, val, v, "solver product, variant %s" % variant)
            if model is not None:
                want = model(v)
                bad = np.flatnonzero(y != want)
                assert same(y, want), ("the device's product is not the model's", variant, len(bad), bad[:5], y[bad[:5]], want[bad[:5]])
            seen[key] = y
        return seen[key].copy()
    return product


def assert_products_reproducible(m, variant, x):
    """Three eager products of x and one replayed from a graph captured on a side stream: the same bytes."""
    first = m.mvp(x, variant=variant)
    for _ in range(2):
        assert m.mvp(x, variant=variant).tobytes() == first.tobytes(), "eager products of one x differ"
    xt = torch.from_numpy(x).cuda()
    yt = torch.zeros(m.n_rows(), dtype=xt.dtype, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            m.mvp_dev(xt.data_ptr(), len(x), yt.data_ptr(), variant, stream=side.cuda_stream)
    yt.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert yt.cpu().numpy().tobytes() == first.tobytes(), "the product replayed from a graph differs from the eager one"


# ---- the solvers -------------------------------------------------------------------------------------------------------------
def run_host(solver, a, b, x0):
    x = x0.copy()
    solver.solve(a, b, x)
    return x


def run_vec(solver, a, b, x0):
    bd, xd = sm.DenseVec.from_vec(b), sm.DenseVec.from_vec(x0)
    solver.solve(a, bd, xd)
    assert same(bd.to_numpy(), b)  # (b is read only)
    return xd.to_numpy()


class Solver:
    """One of the three: the model, the device solves (entry point by entry point) and what is compared."""

    def __init__(self, name):
        self.name = name

    def model(self, off, col, val, b, x0, tol, iter_max, product, fused):
        if self.name == "bicgstab":
            return bm.bicgstab(off, col, val, b, x0, tol, iter_max, product=product)
        return (cg_model.cg if self.name == "cg" else cg_model.pcg)(off, col, val, b, x0, tol, iter_max, fused=fused, product=product)

    def device(self, a, b, x0, tol, iter_max, variant):
        """[(entry point, x, (iterations, f64(rr)[, breakdown, converged]))]"""
        out = []
        if self.name == "pcg":
            runs = [("host", sm.JacobiConjugateGradient(tol, iter_max, variant=variant), run_host)]
        else:
            cls = sm.ConjugateGradient if self.name == "cg" else sm.BiCGStab
            runs = [("vec/%d" % CHECK_EVERY, cls(tol, iter_max, variant=variant, check_every=CHECK_EVERY), run_vec),
                    ("host", cls(tol, iter_max, variant=variant), run_host)]
        for what, s, run in runs:
            x = run(s, a, b, x0)
            scalars = (s.iterations, np.float64(s.r_norm_squared))
            if self.name == "bicgstab":
                scalars += (s.breakdown, s.converged)
            out.append((what, x, scalars))
        return out

    def scalars(self, want):
        if self.name == "bicgstab":
            return want.iterations, np.float64(want.r_norm_squared), want.breakdown, want.converged
        return want.iterations, np.float64(want.r_norm_squared)

    def events(self, want):
        """the norms the stop tests of the bodies saw, in order: [(body, norm)] (BiCGSTAB: the half step's, then the full step's)"""
        if self.name == "bicgstab":
            ev = []
            for k, (ss, rr) in enumerate(zip(want.ss_list, want.rr_list)):
                ev += [(k + 1, math.sqrt(float(ss))), (k + 1, math.sqrt(float(rr)))]
            return ev
        return [(k + 1, math.sqrt(float(rr))) for k, rr in enumerate(want.rr_list)]


SOLVERS = [Solver("cg"), Solver("pcg"), Solver("bicgstab")]


def assert_same_result(solver, got, want, what):
    entry, x, scalars = got
    assert np.isfinite(x).all(), (what, entry, "x is not finite")
    w = solver.scalars(want)
    assert scalars[0] == w[0], (what, entry, "iterations", scalars[0], w[0])
    assert same(scalars[1], w[1]), (what, entry, "r.r", scalars[1], w[1])
    assert scalars[2:] == w[2:], (what, entry, "breakdown, converged", scalars[2:], w[2:])
    bad = np.flatnonzero(x != want.x)
    assert same(x, want.x), (what, entry, "x", len(bad), bad[:5], x[bad[:5]], want.x[bad[:5]])


def stop_tolerance(solver, want):
    """(body k, tol): tol lies strictly between the norm a stop test of body k sees and the smallest norm any earlier stop test
    saw, so the loop has to leave in body k, neither sooner nor later -- k in the middle of a batch of 4 (and of 8)."""
    ev = solver.events(want)
    for k in (6, 7, 10, 3, 2):
        for e, (body, norm) in enumerate(ev):
            if body == k and e and norm < 0.9 * min(v for _, v in ev[:e]):  # (a gap far wider than any rounding of the square root)
                return k, 0.5 * (norm + min(v for _, v in ev[:e]))
    raise AssertionError(("no body in the middle of a batch undercuts all earlier norms", ev))


@pytest.mark.parametrize("name,dtype", CASES)
def test_solvers_equal_the_model_fed_by_the_checked_device_product(gpu, name, dtype):
    cfg = CONFIGS[name]
    off, col, val = cfg.build(dtype)
    n = len(off) - 1
    assert n < 131_072  # (the models' reduction trees at these sizes are pinned by test_cg_bits_gpu.py / test_bicgstab_gpu.py)
    rng = np.random.default_rng(1000 + n)
    b, x0 = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
    a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    fused_env = dict(SMH_CG_FUSED_DOT=None, SMH_STREAM_RPT=None) if cfg.fused else {}
    with env(**cfg.env, **fused_env):
        cfg.knobs(a)
        a.prepare(cfg.variant)
        cfg.check(a)
        assert_products_reproducible(a, cfg.variant, x0)
        product = device_product(a, cfg.variant, off, col, val)
        for solver in SOLVERS:
            want = solver.model(off, col, val, b, x0, 0.0, ITER_MAX, product, cfg.fused)
            assert want.iterations == ITER_MAX and np.isfinite(want.x).all()
            for attempt in ("first solve", "second solve"):
                got = solver.device(a, b, x0, 0.0, ITER_MAX, cfg.variant)
                for g in got:
                    assert_same_result(solver, g, want, (name, solver.name, attempt))
            if cfg.same_as:
                for g in solver.device(a, b, x0, 0.0, ITER_MAX, cfg.same_as):
                    assert_same_result(solver, g, want, (name, solver.name, "as " + cfg.same_as))
            if dtype == cfg.stop or len(cfg.dtypes) == 1:
                k, tol = stop_tolerance(solver, want)
                stopped = solver.model(off, col, val, b, x0, tol, 50, product, cfg.fused)
                assert stopped.iterations == k and not same(stopped.x, solver.model(off, col, val, b, x0, 0.0, k - 1, product, cfg.fused).x)
                for g in solver.device(a, b, x0, tol, 50, cfg.variant):
                    assert_same_result(solver, g, stopped, (name, solver.name, "stop in body %d" % k))
        cfg.check(a)  # (the solves have changed no form)


@pytest.mark.parametrize("name,dtype", CASES)
def test_first_product_builds_what_prepare_builds(gpu, name, dtype):
    """A fresh handle sent straight into a product (the lazy builds inside the first launch) against one that was prepared first: the
    same bytes, the same forms (the configuration's getters) and the same resolution.  The product and smh_crs_prepare read which
    forms a variant runs on from one table (spmv_dispatch.hip); this is the comparison that table could break."""
    cfg = CONFIGS[name]
    n, off, col, val, x = config_matrix(name, dtype)
    with env(**cfg.env):
        prepared = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
        cfg.knobs(prepared)
        prepared.prepare(cfg.variant)
        want = prepared.mvp(x, variant=cfg.variant)
        fresh = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
        cfg.knobs(fresh)
        got = fresh.mvp(x, variant=cfg.variant)
        bad = np.flatnonzero(got != want)
        assert same(got, want), (name, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
        cfg.check(fresh)
        assert fresh.resolved_variant() == prepared.resolved_variant()
