"""SparseMatrix::inner_prod, lhs^T (A rhs), pinned BIT FOR BIT to the CPU models of its three device routes (tests/inner_prod_model.py;
spmv_inner_prod in sparsemat_amd/csrc/spmv_dispatch.hip): K1r's DOT form with its tail slot, the K1s dot epilogue in every form of that
kernel, and the product followed by launch_dot for every kernel without a dot form.  The models are held on the CPU
(tests/test_inner_prod_model.py) to literal walks in exactly rounded arithmetic and to exact sums, and every case here is shown there
to move a bit of its result under each wrong variant of the order it is meant to catch (tests/inner_prod_cases.py: `tells`).

The eight bytes of the result are compared with the model's: no tolerance appears in this file (the one bound used, for the results
with non-finite lhs on empty rows, is the suite's own against the oracle: util.REL_TOL).  Every case goes through both entry points
(host arrays and DenseVecs) and asserts through the handle's getters, before each call, that the route under test is the one that
runs.

Rows WITHOUT entries: the reference reads lhs[i] inside the entry loop, so NaN or Inf there never reaches its sum; the device routes
leave such rows out, and with finite data that changes no bit (test_rows_without_entries_*)."""
import struct

import numpy as np
import pytest

import inner_prod_cases as ipc
import inner_prod_model as ipm
import kernel_forms as kf
import oracle
import sparsemat_amd as sm
from inner_prod_cases import F32, F64
from kernel_forms import env
from sparsemat_amd import _lib
from test_spmv_order_gpu import make_handle
from util import REL_TOL, assert_spmv_close

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]
NO_KNOB = dict(SMH_CG_FUSED_DOT=None, SMH_STREAM_RPT=None, SMH_STREAM_C16=None, SMH_STREAM_XS=None, SMH_STREAM_XD=None, SMH_STREAM_VDICT=None,
               SMH_STREAM_L8=None, SMH_STREAM_SMALL=None, SMH_RING_REGULAR=None, SMH_RING_BLOCKS_PER_CU=None, SMH_RING_WIDE=None,
               SMH_RING_BANDS=None, SMH_GATHER_NT=None)


def packed(v):
    return struct.pack("d", float(v))


def inner_prod_both(m, lhs, x, variant):
    """through the host entry point and through DenseVecs: the same eight bytes"""
    a = m.inner_prod(lhs, x, variant=variant)
    b = m.inner_prod(sm.DenseVec.from_vec(lhs), sm.DenseVec.from_vec(x), variant=variant)
    assert packed(a) == packed(b), (a, b)
    return a


def same_bits(y, want):
    return y.dtype == want.dtype and y.tobytes() == want.tobytes()


# ---- K1r -------------------------------------------------------------------------------------------------------------------------
RING_RUNS = [pytest.param(n, dt, id="%s-%s" % (n, np.dtype(dt).name)) for n, c in ipc.RING_CASES.items() for dt in c.dtypes]


def ring_is_what_runs(m, case, lanes):
    """the plan, asserted: active, the ring and column form the case is about"""
    nb, frac, active, ptr, ph = m.ring_plan()
    assert active and m.resolved_variant()[1] == lanes, (active, m.resolved_variant(), lanes)
    assert (m.ring_entries(), m.ring_bands()) == (case.entries, case.bands)
    if case.form is not None:
        assert m.ring_column_form() == case.form
    assert nb % 8 == 0 and nb + 1 > 256 and len(ptr) == nb + 1  # (threads of launch_fold2's one workgroup fold several partials)
    return nb, ptr, ph


@pytest.mark.parametrize("name,dtype", RING_RUNS)
def test_ring_route(gpu, name, dtype):
    case = ipc.RING_CASES[name]
    n_cols, off, col, val, x = case.build(dtype)
    n_rows, nnz = len(off) - 1, int(off[-1])
    lhs = case.lhs(n_rows, dtype)
    with env(**{**NO_KNOB, **case.env}):
        m = make_handle(n_cols, off, col, val, case.borrowed)
        if case.force:
            m.set_ring(1)
        for lanes, chunks in case.widths:
            m.set_vector_lanes(lanes)
            m.set_vector_chunks(chunks)
            y_ring, tail = ipm.ring_sums(off, col, val, x, lanes, case.borrowed)
            assert (tail is not None) == (case.borrowed and nnz % 4 != 0)
            results = []
            for extra in case.envs:
                with env(**extra):
                    nb, ptr, ph = ring_is_what_runs(m, case, lanes)
                    if "SMH_RING_REGULAR" in extra:  # the body that computes its row offsets, and the one that loads them
                        assert m.ring_regular().any()
                    if case.planned:  # the plan the CPU test showed the case's sensitivity on
                        want_ptr, want_ph = ipm.ring_plan_rows(off, col, nb, case.entries)
                        assert np.array_equal(ptr, want_ptr) and np.array_equal(ph[:, :2], want_ph[:, :2])
                        assert np.array_equal(ph[:, 4] == 1, want_ph[:, 2] == 1)
                    if name == "mixed-phases":
                        assert (ph[:, 4] == 1).any() and (ph[:, 4] != 1).any()
                    if name == "short-rows":
                        assert nb == ipc.RING_BLOCKS and n_rows >= (nb + 1) * 64 and (np.diff(ptr.astype(np.int64)) > 0).sum() > 256
                    want = ipm.ring_route(lhs, y_ring, ptr, ph, lanes, dtype, case.entries, tail)
                    got = inner_prod_both(m, lhs, x, "vector")
                    assert packed(got) == packed(want), (name, lanes, chunks, extra, got, float(want))
                    ring_is_what_runs(m, case, lanes)
                    results.append(got)
                    if not case.planned:  # (no CPU restatement of this plan: the case's sensitivity, on the handle's own)
                        for variant in case.tells:
                            other = ipm.ring_route(lhs, y_ring, ptr, ph, lanes, dtype, case.entries, tail, wrong=(variant,))
                            assert packed(other) != packed(want), (name, variant)
            assert len({packed(r) for r in results}) == 1
        m.set_vector_chunks(0)


# ---- K1s -------------------------------------------------------------------------------------------------------------------------
STREAM_RUNS = [pytest.param(n, dt, id="%s-%s" % (n, np.dtype(dt).name)) for n in ipc.STREAM_CASES for dt in (F32, F64)]


def stream_form_is_what_runs(m, want):
    lay = m.stream_layout()
    assert lay["coded"] == want["coded"] and (lay["xs_chunks"] in (2, 4)) == want["xs"] and lay["xs_chunks"] in (0, 2, 4), lay
    assert m.stream_direct() == want["direct"] and (len(m.stream_value_dict()) > 0) == want["vdict"], (m.stream_direct(), len(m.stream_value_dict()))


@pytest.mark.parametrize("name,dtype", STREAM_RUNS)
def test_stream_route(gpu, name, dtype):
    build, forms, _, seed = ipc.STREAM_CASES[name]
    n_rows, n_cols, off, col, val = build(dtype)
    x, lhs = kf.vector_x(n_cols, dtype, 5), ipc.lhs_vector(n_rows, dtype, seed)
    y = oracle.spmv(off, col, val, x)
    for form in forms:
        form_env, (xs, direct, vdict), want_form = ipc.STREAM_FORMS[form]
        rpt = 2 if form == "rpt2" else 1
        with env(**{**NO_KNOB, **form_env}):
            m = sm.SparseMatCRS.from_raw_parts(n_rows, n_cols, off, col, val)
            m.set_stream_xs(xs)
            m.set_stream_direct(direct)
            m.set_stream_value_dict(vdict)
            m.prepare("stream")
            stream_form_is_what_runs(m, want_form)
            assert same_bits(m.mvp(x, variant="stream"), y), (name, form)  # (K1s is the storage-order product bit for bit)
            want = ipm.stream_route(lhs, y, rpt)
            got = inner_prod_both(m, lhs, x, "stream")
            assert packed(got) == packed(want), (name, form, got, float(want))
            stream_form_is_what_runs(m, want_form)


# ---- every kernel without a dot form -------------------------------------------------------------------------------------------
GENERIC_RUNS = [pytest.param(n, dt, id="%s-%s" % (n, np.dtype(dt).name)) for n in ipc.GENERIC_CASES for dt in (F32, F64)]


@pytest.mark.parametrize("name,dtype", GENERIC_RUNS)
def test_generic_route(gpu, name, dtype):
    build, variants, seed = ipc.GENERIC_CASES[name]
    n_rows, n_cols, off, col, val = build(dtype)
    x, lhs = kf.vector_x(n_cols, dtype, 5), ipc.lhs_vector(n_rows, dtype, seed)
    with env(**{**NO_KNOB, **kf.NO_RING_ENV}):
        m = sm.SparseMatCRS.from_raw_parts(n_rows, n_cols, off, col, val)
        m.set_colblock_shift(8)
        m.set_ring(0)
        for variant in variants:
            if variant == "vector":
                assert not m.ring_plan()[2]  # (K1 without the ring: no DOT form)
            y = m.mvp(x, variant=variant)    # the kernel's own product (pinned to its own model elsewhere), first held to the oracle
            assert_spmv_close(y, off, col, val, x, "%s %s" % (name, variant))
            want = ipm.generic_route(lhs, y)
            got = inner_prod_both(m, lhs, x, variant)
            assert packed(got) == packed(want), (name, variant, got, float(want))
            if variant == "vector":
                assert not m.ring_plan()[2]


# ---- the edges the routes share ------------------------------------------------------------------------------------------------
EDGE_RUNS = [pytest.param(r, dt, id="%s-%s" % (r, np.dtype(dt).name)) for r in ipc.EDGE_ROUTES for dt in (F32, F64)]


class Edge:
    """the matrix with interior and trailing empty rows behind one route: model(lhs) -> the route's model of lhs . (A x)"""

    def __init__(self, route, dtype):
        self.variant, ring, lanes = ipc.EDGE_ROUTES[route]
        self.n_rows, self.n_cols, self.off, self.col, self.val = ipc.empty_rows_matrix(dtype)
        self.x = kf.vector_x(self.n_cols, dtype, 5)
        self.lens = np.diff(self.off.astype(np.int64))
        self.m = m = sm.SparseMatCRS.from_raw_parts(self.n_rows, self.n_cols, self.off, self.col, self.val)
        m.set_ring(ring)
        if lanes:
            m.set_vector_lanes(lanes)
        off, col, val, x = self.off, self.col, self.val, self.x
        if route == "ring":
            nb, _, active, ptr, ph = m.ring_plan()
            assert active and m.resolved_variant()[1] == lanes and m.ring_entries() == 16384 and m.ring_bands() == 1
            y = oracle.spmv_lanes(off, col, val, x, lanes)
            self.model = lambda lhs: ipm.ring_route(lhs, y, ptr, ph, lanes, dtype, 16384)
        elif route == "stream":
            y = oracle.spmv(off, col, val, x)
            assert same_bits(m.mvp(x, variant="stream"), y)
            self.model = lambda lhs: ipm.stream_route(lhs, y)
        else:
            assert not m.ring_plan()[2]
            y = m.mvp(x, variant=self.variant)
            assert_spmv_close(y, off, col, val, x, route)
            self.model = lambda lhs: ipm.generic_route(lhs, y)

    def run(self, lhs):
        return inner_prod_both(self.m, lhs, self.x, self.variant)


@pytest.mark.parametrize("route,dtype", EDGE_RUNS)
def test_short_lhs_and_negative_zeros(gpu, route, dtype):
    """lhs with -0.0, stored -0.0 values and rows whose only product is -0.0 (every accumulator starts at +0: the rows' sums are +0);
    lhs that ends right behind the last row with entries: the full call's bits and the model's with zeros behind; one entry less is
    the reference's panic"""
    with env(**{**NO_KNOB, **kf.NO_RING_ENV}):
        e = Edge(route, dtype)
        lhs = ipc.lhs_vector(e.n_rows, dtype, 6)
        assert np.signbit(lhs[e.lens > 0]).any() and (lhs[e.lens > 0] == 0).any() and np.signbit(e.val[e.val == 0]).any()
        last = int(np.flatnonzero(e.lens)[-1])
        assert last < e.n_rows - 100
        full = e.run(lhs)
        assert packed(full) == packed(e.model(lhs)), (route, full)
        short = e.run(lhs[:last + 1])
        assert packed(short) == packed(full) == packed(e.model(lhs[:last + 1]))
        with pytest.raises(sm.SparseMatPanic) as err:
            e.m.inner_prod(lhs[:last], e.x, variant=e.variant)
        assert err.value.status == _lib.SMH_ERR_INDEX_RANGE
        with pytest.raises(sm.SparseMatPanic) as err:
            e.m.inner_prod(sm.DenseVec.from_vec(lhs[:last]), sm.DenseVec.from_vec(e.x), variant=e.variant)
        assert err.value.status == _lib.SMH_ERR_INDEX_RANGE


@pytest.mark.parametrize("route,dtype", EDGE_RUNS)
def test_rows_without_entries_take_no_part(gpu, route, dtype):
    """lhs finite on every row with entries and NaN / +Inf / -Inf on the interior and trailing rows without: the reference never reads
    those (sparsematrix.rs:165-168).  The result is finite, bit for bit the model's with +0 in their place, and within the suite's
    bound of the oracle's.  NaN on a row WITH entries still gives NaN.
    (On the library before the empty rows were left out this test gave NaN where the reference is finite, in all three routes.)"""
    with env(**{**NO_KNOB, **kf.NO_RING_ENV}):
        e = Edge(route, dtype)
        lhs = ipc.lhs_vector(e.n_rows, dtype, 6)
        empty = np.flatnonzero(e.lens == 0)
        assert ((empty > 1000) & (empty < 1300)).any() and (empty >= e.n_rows - 200).sum() == 200 and (empty < 1000).any()
        special = lhs.copy()
        special[empty] = np.array([np.nan, np.inf, -np.inf], dtype)[np.arange(len(empty)) % 3]
        got = e.run(special)
        assert np.isfinite(got), (route, got)
        assert packed(got) == packed(e.model(ipm.zero_empty_rows(special, e.off))) == packed(e.model(lhs)), (route, got)
        ref = float(oracle.mat_inner_prod(e.off, e.col, e.val, special, e.x))
        scale = float(oracle.mat_inner_prod(e.off, e.col, np.abs(e.val), np.abs(ipm.zero_empty_rows(special, e.off)), np.abs(e.x)))
        assert np.isfinite(ref) and abs(got - ref) <= REL_TOL[np.dtype(dtype)] * scale, (route, got, ref, scale)
        control = lhs.copy()
        control[int(np.flatnonzero(e.lens)[5])] = np.nan
        assert np.isnan(e.run(control)), route


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_rows_and_no_entries_give_zero(gpu, dtype):
    """n_rows == 0, and nnz == 0 with NaN in lhs: +0.0, whichever kernel is asked for"""
    x = kf.vector_x(5, dtype)
    for n_rows in (0, 7):
        m = sm.SparseMatCRS.from_raw_parts(n_rows, 5, np.zeros(n_rows + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype))
        lhs = np.full(n_rows, np.nan, dtype)
        for variant, ring in (("vector", 1), ("vector", 0), ("stream", 0), ("seq", 0), ("merge", 0), ("auto", -1)):
            m.set_ring(ring)
            assert packed(inner_prod_both(m, lhs, x, variant)) == packed(0.0), (n_rows, variant)
