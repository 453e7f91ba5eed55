"""GPU: the non-symmetric factorized sparse approximate inverse (smh_crs_fsai_ns: csrc/fsai.hip) and its application
(smh_crs_fsai_ns_apply_vec) pinned BIT FOR BIT to tests/fsai_ns_model.py: G_L, G_U (offsets, columns, values) and `singular` on the
cases of tests/fsai_ns_cases.py (which tests/test_fsai_ns_model.py shows to move a bit under each wrong variant), at every lane width
and on both sides of the LDS-to-scratch switch (fsai_ns_cases.fit(lanes)); the refusals and statuses, with the outputs left alone;
the application against the device's own products of gl and gu, each held to the suite's parity bound first; the factors as
ordinary handles."""
import ctypes as C

import numpy as np
import pytest

import bicgstab_model as bm
import fsai_ns_cases as nc
import fsai_ns_model as nm
import sparsemat_amd as sm
import trisolve_model as tm
from kernel_forms import same
from sparsemat_amd import _lib
from test_solver_kernels_gpu import device_product

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPES = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]


def handle(off, col, val, validate=True):
    n = len(off) - 1
    return sm.SparseMatCRS.from_raw_parts(n, n, off, col, val, validate=validate)


def status_of(call):
    with pytest.raises(_lib.SparseMatPanic) as e:
        call()
    return e.value.status, str(e.value)


def assert_pair(gl, gu, want_l, want_u, what, by_class=False):
    """gl and gu against the model's (off, col, val): offsets and columns equal, values bit for bit (by_class: bits where the model is
    finite, the class elsewhere)."""
    n = len(want_l[0]) - 1
    for h, (o, c, v), name in ((gl, want_l, "gl"), (gu, want_u, "gu")):
        ho, hc, hv = h.raw_parts()
        assert h.n_rows() == n and h.dtype == v.dtype and (n == 0 or h.n_cols() == n), (what, name)
        assert np.array_equal(ho, o) and np.array_equal(hc, c), (what, name, "pattern")
        if by_class:
            fin = np.isfinite(v)
            assert same(hv[fin], v[fin]) and np.array_equal(np.isnan(hv), np.isnan(v)) and np.array_equal(hv[np.isinf(v)], v[np.isinf(v)]), (what, name)
        else:
            bad = np.flatnonzero(hv != v)
            assert same(hv, v), (what, name, len(bad), bad[:5], hv[bad[:5]], v[bad[:5]])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(nc.NAMES))
def test_factors_equal_the_model(gpu, name, dtype):
    off, col, val = nc.matrix(name, dtype)
    want_l, want_u, want_bad = nc.factor(name, dtype)
    a = handle(off, col, val)
    gl, gu, bad = a.fsai_ns()
    assert bad is None and want_bad is None
    assert_pair(gl, gu, want_l, want_u, name)
    assert same(a.raw_parts()[2], val)  # (the matrix itself is untouched)
    lens_l, lens_u = np.diff(want_l[0].astype(np.int64)), np.bincount(want_u[1], minlength=len(off) - 1)  # (a row of H is a column of G_U)
    if name in ("empty", "one", "diagonal"):
        assert len(lens_l) < 2 or (lens_l.max() == 1 and lens_u.max() == 1)
        return
    # which form a case runs in (the lanes are the mean row's of each factor): the long-row route is taken where the cases say
    hoff = np.concatenate([[0], np.cumsum(lens_u)])
    long_l, long_u = (lens_l > nc.fit(nc.auto_lanes(want_l[0]))).sum(), (lens_u > nc.fit(nc.auto_lanes(hoff))).sum()
    assert (long_l > 0) == (name in ("dense70", "ragged", "arrow_row128")), (name, long_l)
    assert long_u > 0 or name not in ("dense70", "arrow_col128"), (name, long_u)  # (random upper patterns have a few long columns too)
    assert long_l < len(lens_l) and long_u < len(lens_u)
    if name == "arrow_row128":
        assert lens_l.max() == nc.MAX_ROW
    if name == "arrow_col128":
        assert lens_u.max() == nc.MAX_ROW


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ragged", "dense70", "random_ns", "convdiff12"])
def test_every_lane_width_gives_the_same_bits(gpu, name, dtype):
    """ragged has every m from 1 to 128 twice in G_L: for every lane width L the rows of m = L, L + 1 and 2 L + 1 (one, two and three
    trips of the group over the square's rows) and of m = fit(L) and fit(L) + 1 (the last row in the LDS, the first in scratch)."""
    off, col, val = nc.matrix(name, dtype)
    want_l, want_u, _ = nc.factor(name, dtype)
    lens = set(np.diff(want_l[0].astype(np.int64)).tolist())
    a = handle(off, col, val)
    for lanes in nc.LANES:
        if name == "ragged":
            assert {lanes, lanes + 1, min(2 * lanes + 1, 128), nc.fit(lanes), nc.fit(lanes) + 1} <= lens
        a.set_vector_lanes(lanes)
        gl, gu, bad = a.fsai_ns()
        assert bad is None
        assert_pair(gl, gu, want_l, want_u, (name, lanes))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(nc.REFUSED))
def test_rows_and_columns_beyond_the_limit_are_refused(gpu, name, dtype):
    what, where = nc.REFUSED[name]
    a = handle(*nc.matrix(name, dtype))
    st, msg = status_of(a.fsai_ns)
    assert st == _lib.SMH_ERR_INVALID and "%s %d " % (what, where) in msg and str(nc.MAX_ROW) in msg
    gl, gu, bad = C.c_void_p(), C.c_void_p(), C.c_size_t(7)
    assert sm.lib().smh_crs_fsai_ns(a._h, C.byref(gl), C.byref(gu), C.byref(bad)) == _lib.SMH_ERR_INVALID
    assert gl.value is None and gu.value is None and bad.value == 7


@pytest.mark.parametrize("dtype", DTYPES)
def test_singular_and_non_finite_values(gpu, dtype):
    # a block (1 2; 2 4) in rows 2 and 3 of a diagonal matrix: the last pivot of row 3 -- and of column 3 -- is 4 - 2 * 2 = 0
    rows = [[(0, 4.0)], [(1, 9.0)], [(2, 1.0), (3, 2.0)], [(2, 2.0), (3, 4.0)], [(4, 16.0)]]
    off, col, val = tm.from_rows(rows, dtype)
    want_l, want_u, want_bad = nm.fsai_ns(off, col, val)
    gl, gu, bad = handle(off, col, val).fsai_ns()
    assert bad == want_bad == 3 and np.isinf(want_u[2]).sum() == 2
    assert_pair(gl, gu, want_l, want_u, "zero pivot", by_class=True)
    assert gl.raw_parts()[2].tolist() == [1, 1, 1, -2, 1, 1]
    # a zero pivot in a row of one: 1 / 0 is +Inf in G_U, and the row is reported
    gl, gu, bad = handle(*tm.from_rows([[(0, 1.0)], [(1, 0.0)]], dtype)).fsai_ns()
    assert bad == 1 and gl.raw_parts()[2].tolist() == [1.0, 1.0] and gu.raw_parts()[2].tolist() == [1.0, np.inf]
    # a stored NaN and a stored Inf: bits where the model is finite, the class elsewhere
    off, col, val = nc.matrix("random_ns", dtype)
    val = val.copy()
    pos = tm.diag_positions(off, col)
    val[pos[40] - 1] = np.nan
    val[pos[120]] = np.inf
    want_l, want_u, want_bad = nm.fsai_ns(off, col, val)
    assert want_bad == 40 and np.isnan(want_l[2]).any() and np.isnan(want_u[2]).any()
    for lanes in (0, 1, 64):
        a = handle(off, col, val)
        if lanes:
            a.set_vector_lanes(lanes)
        gl, gu, bad = a.fsai_ns()
        assert bad == want_bad
        assert_pair(gl, gu, want_l, want_u, ("non-finite", lanes), by_class=True)
    # the Inf alone: every value is finite (x / Inf = 0) and the row is still named
    val = nc.matrix("random_ns", dtype)[2].copy()
    val[pos[120]] = np.inf
    want_l, want_u, want_bad = nm.fsai_ns(off, col, val)
    gl, gu, bad = handle(off, col, val).fsai_ns()
    assert bad == want_bad == 120 and np.isfinite(want_u[2]).all()
    assert_pair(gl, gu, want_l, want_u, "Inf on the diagonal")


def test_statuses(gpu):
    L = sm.lib()

    def refused(a):
        gl, gu, bad = C.c_void_p(), C.c_void_p(), C.c_size_t(7)
        st = L.smh_crs_fsai_ns(a._h, C.byref(gl), C.byref(gu), C.byref(bad))
        assert gl.value is None and gu.value is None and bad.value == 7  # nothing is made
        return st, L.smh_last_error().decode()

    st, msg = refused(handle(*tm.from_rows([[(0, 1.0)], [(1, 1.0)], [(2, 1.0), (0, 1.0)], [(3, 1.0), (1, 1.0)]], F32)))
    assert st == _lib.SMH_ERR_INVALID and "row 2" in msg and "ascending" in msg
    st, msg = refused(handle(*tm.from_rows([[(0, 1.0)], [(0, 1.0), (1, 1.0), (1, 1.0)]], F32)))
    assert st == _lib.SMH_ERR_INVALID and "row 1" in msg and "ascending" in msg
    st, msg = refused(handle(*tm.from_rows([[(0, 1.0)], [(1, 1.0)], [(0, 1.0)], [(0, 1.0), (2, 1.0)]], F32)))
    assert st == _lib.SMH_ERR_INVALID and "row 2" in msg and "diagonal" in msg
    orphan = sm.SparseMatCRS.from_triplets([1, 0, 1, 0], [1, 0, 0, 1], np.ones(4, F32), into_crs=True)
    assert orphan.orphans() == 1
    st, msg = refused(orphan)
    assert st == _lib.SMH_ERR_INVALID and "orphan" in msg
    rect = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 1, 2], [0, 1], np.ones(2, F32))
    assert refused(rect)[0] == _lib.SMH_ERR_NOT_SQUARE
    wide = sm.SparseMatCRS.from_raw_parts(2, 2, [0, 1, 3], [0, 1, 5], np.ones(3, F32), validate=False)
    assert refused(wide)[0] == _lib.SMH_ERR_INDEX_RANGE
    both = sm.SparseMatCRS.from_raw_parts(2, 3, [0, 2, 3], [1, 0, 1], np.ones(3, F32))  # the contract's order: not square before unsorted
    assert refused(both)[0] == _lib.SMH_ERR_NOT_SQUARE
    # NULL pointers; singular_out may be NULL
    good = handle(*nc.matrix("random_ns", F32))
    want_l, want_u, _ = nc.factor("random_ns", F32)
    gl, gu, bad = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert L.smh_crs_fsai_ns(None, C.byref(gl), C.byref(gu), C.byref(bad)) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_fsai_ns(good._h, None, C.byref(gu), C.byref(bad)) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_fsai_ns(good._h, C.byref(gl), None, C.byref(bad)) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_fsai_ns(good._h, C.byref(gl), C.byref(gu), None) == _lib.SMH_OK and gl.value and gu.value
    glm, gum = sm.SparseMatCRS(gl, F32), sm.SparseMatCRS(gu, F32)
    assert_pair(glm, gum, want_l, want_u, "singular_out NULL")
    # the application's statuses: smh_crs_fsai_apply_vec's
    n = good.n_rows()
    r, z = sm.DenseVec.zeros(n, F32), sm.DenseVec.zeros(n, F32)
    for args in ((None, gum._h, r._h, z._h), (glm._h, None, r._h, z._h), (glm._h, gum._h, None, z._h), (glm._h, gum._h, r._h, None)):
        assert L.smh_crs_fsai_ns_apply_vec(*args) == _lib.SMH_ERR_INVALID
    assert L.smh_crs_fsai_ns_apply_vec(glm._h, gum._h, r._h, sm.DenseVec.zeros(n, F64)._h) == _lib.SMH_ERR_INVALID
    assert status_of(lambda: glm.fsai_ns_apply(gum, np.zeros(n - 1, F32)))[0] == _lib.SMH_ERR_DIM_MISMATCH
    assert status_of(lambda: rect.fsai_ns_apply(gum, np.zeros(2, F32)))[0] == _lib.SMH_ERR_NOT_SQUARE
    small = handle(*tm.from_rows([[(0, 2.5), (1, -0.7)], [(0, -0.7), (1, 3.1)]], F32))
    assert status_of(lambda: glm.fsai_ns_apply(small, np.zeros(n, F32)))[0] == _lib.SMH_ERR_DIM_MISMATCH
    g64 = handle(*[x if i < 2 else x.astype(F64) for i, x in enumerate(gum.raw_parts())])
    assert status_of(lambda: glm.fsai_ns_apply(g64, np.zeros(n, F32)))[0] == _lib.SMH_ERR_INVALID
    assert status_of(lambda: orphan.fsai_ns_apply(orphan, np.zeros(2, F32)))[0] == _lib.SMH_ERR_INVALID


def test_empty_one_and_hand_case(gpu):
    for dtype in (F32, F64):
        z = handle(*nc.matrix("empty", dtype))
        gl, gu, bad = z.fsai_ns()
        assert gl.n_rows() == 0 and gu.n_rows() == 0 and gl.n_non_zero_entries() == 0 and bad is None
        assert len(gl.fsai_ns_apply(gu, np.zeros(0, dtype))) == 0
        gl, gu, bad = handle(*tm.from_rows([[(0, 4.0)]], dtype)).fsai_ns()
        assert gl.raw_parts()[2].tolist() == [1.0] and gu.raw_parts()[2].tolist() == [0.25] and bad is None
        assert gl.fsai_ns_apply(gu, [10.0]).tolist() == [2.5]
        # A = L U with L = (1; 2 1; 4 3 1), U = (2 1 1; 0 1 1; 0 0 2): G_L = L^-1 and G_U = U^-1, every step exact
        a = handle(*bm.dense_to_crs([[2, 1, 1], [4, 3, 3], [8, 7, 9]], dtype))
        gl, gu, bad = a.fsai_ns()
        assert bad is None and gl.raw_parts()[2].tolist() == [1, -2, 1, 2, -3, 1]
        assert gu.raw_parts()[1].tolist() == [2, 1, 0, 2, 1, 2] and same(gu.raw_parts()[2], np.array([-0.0, -0.5, 0.5, -0.5, 1, 0.5], dtype))
        assert gl.fsai_ns_apply(gu, a.mvp(np.array([1, -2, 3], dtype))).tolist() == [1, -2, 3]


# ---- the application and the handles -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["tridiag3000", "dense70", "random_ns", "convdiff24"])
def test_apply_equals_the_products(gpu, name, dtype):
    off, col, val = nc.matrix(name, dtype)
    want_l, want_u, _ = nc.factor(name, dtype)
    n = len(off) - 1
    gl, gu, _ = handle(off, col, val).fsai_ns()
    r = tm.awkward(np.random.default_rng(n), n, dtype)
    first, second = device_product(gl, "auto", *want_l), device_product(gu, "auto", *want_u)
    want = second(first(r))
    assert np.isfinite(want).all() and want.any()
    got = gl.fsai_ns_apply(gu, r)
    assert same(got, want), np.flatnonzero(got != want)[:5]
    rd = sm.DenseVec.from_vec(r)
    assert same(gl.fsai_ns_apply(gu, rd).to_numpy(), want) and same(rd.to_numpy(), r)  # out of place
    assert gl.fsai_ns_apply(gu, rd, out=rd) is rd and same(rd.to_numpy(), want)          # in place: z may be r
    assert same(gl.fsai_apply(gu, r), want)                                              # (the same entry point under its first name)
    # the factors are ordinary handles: clone, download, single entries, products by any kernel
    assert same(gl.clone().raw_parts()[2], want_l[2]) and same(gu.clone().raw_parts()[2], want_u[2])
    rows = np.arange(n, dtype=np.uint32)
    assert (np.asarray(gl.get_many(rows, rows)) == 1).all()
    assert same(np.asarray(gu.get_many(rows, rows)), want_u[2][want_u[0][1:].astype(np.int64) - 1])  # (descending: the diagonal is a row's last)
    assert same(device_product(gu, "seq", *want_u)(r), gu.mvp(r, variant="seq"))
    assert gl.n_non_zero_entries() == len(want_l[1]) and gu.n_non_zero_entries() == len(want_u[1]) and gu.orphans() == 0
