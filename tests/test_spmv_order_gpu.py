"""The lane-group kernels K1 (spmv_vector.hip) and K1r (spmv_ring2.hip) and the merge-path kernel K2 (spmv_merge.hip) pinned BIT FOR BIT,
in every row of every product, to the oracle's CPU models of their summation orders (oracle.spmv_lanes, oracle.spmv_merge).  The
models are held on the CPU (tests/test_spmv_order_model.py) to a pure-Python restatement with exactly rounded arithmetic, to the
reference's storage-order sum within the suite's parity bound on every matrix launched here, and shown to change bits under every
wrong variant of the order (another chunk grid, lane layout, width, butterfly, FMA or not; other tiles, carry order, association).
No tolerance appears in this file.  The form under test is asserted through the handle's getters before and after each product.

K1 against K1r on borrowed, unpadded arrays: the ring kernel streams whole 16-byte chunks only and a one-thread kernel appends
the last nnz mod 4 entries to their rows' stored results (tail_from = nnz & ~3), where K1 gives those entries to the lanes that own
their slots.  On the ragged matrix the two models differ in ONE row, the last one (row 4100, 37 + nnz mod 4 entries from s mod 4 ==
2: the only row with entries from nnz & ~3 on), at 8 and more lanes (f32, nnz mod 4 == 2: from 4 lanes; nnz mod 4 == 3: only f64 at
8 lanes); with 1 and 2 lanes they agree everywhere.  Each kernel is compared with its own model.  The row-partitioned product
sends a block's boundary rows through K1 and its interior rows through K1r: for a block ADOPTED from borrowed, unpadded arrays
(smh_par_adopt) the block's last rows are boundary rows whenever there are any, so with the overlap on they take K1's bits and
with it off K1r's with the tail -- the two modes can differ there in the last bit; blocks the partition
creates itself own padded arrays and have no tail."""
import numpy as np
import pytest

import kernel_forms as kf
import oracle
import sparsemat_amd as sm
from kernel_forms import CONFIGS, F32, F64, LANES, env, same
from sparsemat_amd import synth

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]


def make_handle(n_cols, off, col, val, borrowed):
    """an owned (padded) copy, or borrowed device arrays of exactly nnz entries"""
    n_rows = len(off) - 1
    if not borrowed:
        return sm.SparseMatCRS.from_raw_parts(n_rows, n_cols, off, col, val)
    bo, bc, bv = synth.DeviceBuffer(off.nbytes), synth.DeviceBuffer(max(col.nbytes, 4)), synth.DeviceBuffer(max(val.nbytes, 8))
    bo.upload(off)
    if len(val):
        bc.upload(col)
        bv.upload(val)
    return sm.SparseMatCRS.from_device_parts(n_rows, n_cols, len(val), bo.ptr, bc.ptr, bv.ptr, val.dtype.type, keep=(bo, bc, bv))


def assert_rows_equal(y, want, what):
    bad = np.flatnonzero(y != want)
    assert same(y, want), (what, "%d rows differ" % len(bad), bad[:5], y[bad[:5]], want[bad[:5]])


# ---- the lane-group family ---------------------------------------------------------------------------------------------------
RAGGED_FORMS = [("owned", 3, False)] + [("borrowed-nnz%d" % mod, mod, True) for mod in range(4)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,nnz_mod,borrowed", RAGGED_FORMS, ids=[f[0] for f in RAGGED_FORMS])
def test_ragged_rows_through_k1_and_k1r(gpu, form, nnz_mod, borrowed, dtype):
    """Every row length 0 ... 9, 4L - 1, 4L, 4L + 1, 8L + 1 for every L, 515, at every start s mod 4, a run of 321 empty rows, 4101
    rows: K1 at every width, K1r at every width and at 2 and 3 chunks per lane.  Owned arrays (nnz mod 4 == 3, padded: no tail) and
    borrowed, unpadded ones with nnz mod 4 = 0 ... 3 (K1r: the model with tail_from)."""
    n_cols, off, col, val = kf.ragged(dtype, nnz_mod)
    x = kf.vector_x(n_cols, dtype)
    nnz = int(off[-1])
    assert nnz % 4 == nnz_mod and all((len(off) - 1) % (8 * (256 // lanes)) for lanes in LANES)
    tail = (nnz & ~3) if borrowed else None
    with env(**kf.NO_RING_ENV):
        m = make_handle(n_cols, off, col, val, borrowed)
        for lanes in LANES:
            want = oracle.spmv_lanes(off, col, val, x, lanes)
            m.set_ring(0)
            m.set_vector_lanes(lanes)
            assert m.resolved_variant()[1] == lanes and not m.ring_plan()[2]
            assert_rows_equal(m.mvp(x, variant="vector"), want, ("K1", form, lanes))
            assert m.resolved_variant()[1] == lanes and not m.ring_plan()[2]
        for lanes, chunks in [(lanes, 0) for lanes in LANES] + [(1, 2), (1, 3), (2, 2)]:
            want = oracle.spmv_lanes(off, col, val, x, lanes, tail_from=tail)  # (the chunks per lane do not change the order)
            m.set_ring(1)
            m.set_vector_lanes(lanes)
            m.set_vector_chunks(chunks)
            plan = m.ring_plan()
            assert m.resolved_variant()[1] == lanes and plan[2] and (plan[4][:, 4] == 1).any()  # (K1r, and rows served from the ring)
            assert_rows_equal(m.mvp(x, variant="vector"), want, ("K1r", form, lanes, chunks))
            assert m.resolved_variant()[1] == lanes and m.ring_plan()[2]
        m.set_vector_chunks(0)


VECTOR_CASES = [pytest.param(name, dt, id="%s-%s" % (name, "f32" if dt == F32 else "f64"))
                for name in kf.vector_config_names() for dt in CONFIGS[name].dtypes]


@pytest.mark.parametrize("name,dtype", VECTOR_CASES)
def test_vector_forms_of_the_solver_configurations(gpu, name, dtype):
    """every vector-family entry of CONFIGS (K1 at 1, 8 and 32 lanes; K1r by column form, on the wide and on the banded ring; what
    AUTO takes), at its size there, in the form its check asserts"""
    cfg = CONFIGS[name]
    n_cols, off, col, val, x = kf.config_matrix(name, dtype)
    with env(**cfg.env):
        m = sm.SparseMatCRS.from_raw_parts(len(off) - 1, n_cols, off, col, val)
        cfg.knobs(m)
        m.prepare(cfg.variant)
        cfg.check(m)
        family, lanes = m.resolved_variant()  # (what AUTO would take, and the lanes of the vector family)
        assert cfg.variant == "vector" or (cfg.variant, family) == ("auto", "vector")
        assert lanes == kf.VECTOR_CONFIG_LANES[name]  # (the width the CPU tests took this case at)
        assert_rows_equal(m.mvp(x, variant=cfg.variant), oracle.spmv_lanes(off, col, val, x, lanes), name)
        cfg.check(m)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_ring_and_gather_phases(gpu, dtype):
    """one K1r plan with ring phases, restarts and global-gather phases (the generator of test_ring_gpu.py's mixed-phase test)"""
    n_cols, off, col, val, x = kf.mixed_phases(dtype)
    with env(**kf.NO_RING_ENV):
        m = sm.SparseMatCRS.from_raw_parts(len(off) - 1, n_cols, off, col, val)
        for lanes in (2, 8):
            m.set_vector_lanes(lanes)
            m.set_ring(1)
            for when in ("before", "after"):
                nb, frac, active, ptr, ph = m.ring_plan()
                assert active and m.resolved_variant()[1] == lanes and (ph[:, 4] == 1).any() and (ph[:, 4] != 1).any() and 0.5 < frac < 1.0, when
                if when == "before":
                    assert_rows_equal(m.mvp(x, variant="vector"), oracle.spmv_lanes(off, col, val, x, lanes), ("mixed", lanes))


# ---- merge -------------------------------------------------------------------------------------------------------------------
MERGE_RUNS = [(name, False) for name in kf.MERGE_CASES] + [(name, True) for name in kf.MERGE_BORROWED]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,borrowed", MERGE_RUNS, ids=["%s%s" % (n, "-borrowed" if b else "") for n, b in MERGE_RUNS])
def test_merge_path_rows(gpu, name, borrowed, dtype):
    build, crossings = kf.MERGE_CASES[name]
    n_cols, off, col, val = build(dtype)
    x = kf.vector_x(n_cols, dtype)
    n_rows, nnz = len(off) - 1, len(val)
    m = make_handle(n_cols, off, col, val, borrowed)
    m.prepare("merge")

    def check_form():
        rows, nz, tile = m.merge_table()
        n_tiles = (n_rows + nnz + tile - 1) // tile
        assert tile == oracle.MERGE_TILE and len(rows) - 1 == n_tiles and (n_tiles == 1) == (name == "single-tile")
        want_rows, want_nz = oracle.merge_path_search(off, nnz, np.arange(n_tiles + 1, dtype=np.uint64) * tile)
        assert np.array_equal(rows, want_rows) and np.array_equal(nz, want_nz)

    check_form()
    assert int(kf.merge_crossings(off).max()) >= crossings
    if borrowed:
        assert nnz % 4  # (the arrays end inside a 16-byte chunk)
    assert_rows_equal(m.mvp(x, variant="merge"), oracle.spmv_merge(off, col, val, x), (name, borrowed))
    check_form()
