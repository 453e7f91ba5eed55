"""Non-finite data and gradual underflow through every SpMV kernel form.

The reference loop (y_i = sum_j a_ij x_j, one rounded multiply and one rounded add per entry, from +0) has well-defined results
for such data: a non-finite x_j reaches exactly the rows that reference column j, a stored zero times Inf is NaN, every other row
is what it would have been, and sums of subnormal products are kept.  The kernels are built from the constructions where this
goes wrong quietly -- padded chunks, loads of zeros past a descriptor, products written for slots nobody owns, clamped columns
masked with selects, segmented scans and carries, LDS stages of x holding columns a tile's rows do not reference, a value
dictionary picked by code bits -- and a mask by multiplication or a scan that subtracts a prefix is right on finite data only.

Every input is seeded and built in tests/special_model.py, where the CPU tests hold the same data against the oracle; all
structure is well-formed (nothing here can fault a kernel, only the floating-point data is unusual).  Each case asserts through
the handle's introspection that the form it names really ran.  Checked per form: the parity gate (finite rows within the bound,
the others of the oracle's class), for SEQ and the K1s family the oracle's bits on finite rows, the fused lhs . (A x), the
device path into a y pre-filled with a NaN pattern (every row overwritten, empty rows exactly +0), run-to-run bit equality."""
import functools
import os

import numpy as np
import pytest

import oracle
import sparsemat_amd as sm
import special_model as sp
from sparsemat_amd import synth
from util import REL_TOL, assert_spmv_close, value_class

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
FILL = {np.dtype(np.float32): (np.uint32, 0x7FC12345), np.dtype(np.float64): (np.uint64, 0x7FF8000012345678)}  # what y holds before mvp_dev


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    """Bit equality but for the sign and payload of NaNs (two kernels may multiply in another operand order: another NaN)."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


class Case:
    """One matrix with its special-value inputs, the oracle's results and the model's classes: computed once, never written to."""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, np.dtype(dtype)
        self.n_rows, self.n_cols, self.off, self.col, self.val, self.share = sp.matrix(name, dtype)
        self.lens = np.diff(self.off.astype(np.int64))
        self.inputs = []
        for tag, val, x in sp.inputs(name, dtype):
            y_ref = oracle.spmv(self.off, self.col, val, x)
            cls = sp.row_classes(self.off, self.col, val, x)
            fin = sp.finite_share(self.off, cls)
            # conditions on the INPUT, asserted on the model before any launch
            assert np.array_equal(cls, value_class(y_ref)), (name, tag)
            assert (0.2 <= fin <= 0.8) if tag == "x_sparse" else (0.0 < fin < 1.0), (name, tag, fin)
            for a in (val, x, y_ref, cls):
                a.setflags(write=False)
            self.inputs.append((tag, val, x, y_ref, cls))
        self.val_special = self.inputs[2][1]
        assert all(np.array_equal(bits(v), bits(self.val_special if tag.startswith("val_special") else self.val)) for tag, v, _, _, _ in self.inputs)
        for a in (self.off, self.col, self.val):
            a.setflags(write=False)

    def handles(self, configure=None):
        """A handle per value array (plain, special), each configured the same way."""
        out = {}
        for key, val in (("plain", self.val), ("special", self.val_special)):
            m = sm.SparseMatCRS.from_raw_parts(self.n_rows, self.n_cols, self.off, self.col, val)
            if configure is not None:
                configure(m)
            out[key] = m
        return out

    def runs(self, handles):
        for tag, val, x, y_ref, cls in self.inputs:
            yield handles["special" if tag.startswith("val_special") else "plain"], tag, val, x, y_ref, cls


@functools.lru_cache(maxsize=None)
def case(name, dtname):
    return Case(name, np.dtype(dtname).type)


def check_y(c, y, tag, val, x, y_ref, cls, what, exact):
    what = "%s %s %s %s" % (c.name, c.dtype.name, tag, what)
    assert y.dtype == c.dtype and y.shape == (c.n_rows,), what
    assert_spmv_close(y, c.off, c.col, val, x, what)
    assert np.array_equal(value_class(y), cls), what                       # (the gate has said so already; the model says it again)
    assert not bits(y[c.lens == 0]).any(), what + ": an empty row is exactly +0"
    if exact:
        fin = cls == 0
        assert np.array_equal(bits(y[fin]), bits(y_ref[fin])), what + ": finite rows bit for bit the oracle's (%d differ)" % (bits(y[fin]) != bits(y_ref[fin])).sum()


def device_path(m, c, x, variant):
    """mvp_dev into a y that holds a NaN pattern: returns what y holds afterwards."""
    u, pat = FILL[c.dtype]
    xbuf = synth.DeviceBuffer(len(x) * c.dtype.itemsize)
    xbuf.upload(x)
    ybuf = synth.DeviceBuffer(c.n_rows * c.dtype.itemsize)
    ybuf.upload(np.full(c.n_rows, pat, u))
    m.mvp_dev(xbuf.ptr, len(x), ybuf.ptr, variant)
    sm.lib().smh_device_synchronize()
    y = ybuf.download(c.dtype, c.n_rows)
    assert not (bits(y) == u(pat)).any(), "rows that were not overwritten"
    return y


def check_inner_prod(m, c, variant, tag, val, x, y_ref, cls, what):
    """Fused lhs . (A x): finite iff the oracle's is, and then within the bound of test_matrix_inner_prod; else the same class."""
    rng = np.random.default_rng(len(what) + c.n_rows)
    lhs_random = rng.uniform(-1, 1, c.n_rows).astype(c.dtype)
    with np.errstate(invalid="ignore"):
        toward = np.where(cls == 2, -0.5, 0.5).astype(c.dtype)             # +Inf rows times +0.5, -Inf rows times -0.5
    lhs_signed = np.where(cls != 0, toward, lhs_random).astype(c.dtype)
    lhs_zero = np.where(cls != 0, 0, lhs_random).astype(c.dtype)          # zero on the non-finite rows: 0 * Inf = NaN in the reference too
    for name, lhs in (("random", lhs_random), ("signed", lhs_signed), ("zero on non-finite rows", lhs_zero)):
        want = sp.dot_class(lhs, y_ref)
        got = m.inner_prod(lhs, x, variant=variant)
        assert value_class(np.array([got]))[0] == want, (what, tag, name, got, want)
        assert want != 0                                                   # (these inputs always leave a non-finite row)
    assert sp.dot_class(lhs_zero, y_ref) == 3


def check_inner_prod_finite(m, c, variant, what):
    rng = np.random.default_rng(c.n_rows)
    lhs, x = rng.uniform(-1, 1, c.n_rows).astype(c.dtype), sp.x_finite(1, c.n_cols, c.dtype.type)
    ref = float(oracle.mat_inner_prod(c.off, c.col, c.val, lhs, x))
    scale = float(oracle.mat_inner_prod(c.off, c.col, np.abs(c.val), np.abs(lhs), np.abs(x)))
    got = m.inner_prod(lhs, x, variant=variant)
    assert abs(got - ref) <= REL_TOL[c.dtype] * scale, (what, got, ref, scale)


def sweep(c, handles, variant, what, exact=False, inner_prod=False):
    """Every special-value input through one configured form."""
    first = True
    for m, tag, val, x, y_ref, cls in c.runs(handles):
        y = m.mvp(x, variant=variant)
        check_y(c, y, tag, val, x, y_ref, cls, what, exact)
        if first or tag == "val_special+x_sparse":
            assert np.array_equal(bits(y), bits(m.mvp(x, variant=variant))), what + ": run-to-run"
        if tag in ("x_single", "val_special+x_sparse"):                    # the device path, once per value array
            y_dev = device_path(m, c, x, variant)
            check_y(c, y_dev, tag, val, x, y_ref, cls, what + " (mvp_dev)", exact)
            assert np.array_equal(bits(y_dev), bits(y)), what + ": mvp_dev = mvp"
        if inner_prod:
            check_inner_prod(m, c, variant, tag, val, x, y_ref, cls, what)
        first = False
    if inner_prod:
        check_inner_prod_finite(handles["plain"], c, variant, what)


def with_env(name, flag, fn):
    """fn() with the knob set; what the variable held before (a suite run under a global knob) is put back."""
    before = os.environ.get(name)
    try:
        os.environ[name] = flag
        return fn()
    finally:
        if before is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = before


# ---- SEQ, K1s, K2 merge, K1 / K1r at every lane width, AUTO ---------------------------------------------------------------------
@DTYPES
def test_basic_forms(gpu, dtype):
    c = case("ragged3001", np.dtype(dtype).name)
    assert c.lens.max() == 5000 and (c.lens == 2600).any() and (c.lens == 0).any()
    h = c.handles()
    sweep(c, h, "seq", "seq", exact=True)
    for m in h.values():   # rows of 2600 and 5000 entries: tiles beyond the LDS stage -> no small single-pass tiles, the multi-pass path
        lay = m.stream_layout()
        assert not lay["small_tiles"] and not lay["byte_lengths"] and lay["xs_chunks"] == 0, lay
    sweep(c, h, "stream", "stream", exact=True, inner_prod=True)
    sweep(c, h, "merge", "merge", inner_prod=True)
    for lanes in (1, 4, 8, 64):
        for ring in (1, 0):
            for m in h.values():
                m.set_vector_lanes(lanes)
                m.set_ring(ring)
                assert m.ring_plan()[2] == bool(ring), (lanes, ring)
            sweep(c, h, "vector", "vector lanes %d ring %d" % (lanes, ring), inner_prod=(lanes == 4))
    for m in h.values():
        m.set_vector_lanes(0)
        m.set_ring(-1)
    for m in h.values():
        assert m.resolved_variant()[0] == "merge"                            # what AUTO runs on this skewed matrix
    sweep(c, h, "auto", "auto (merge)", inner_prod=True)


@DTYPES
def test_stream_on_borrowed_unpadded_arrays(gpu, dtype):
    """Device arrays that end with their last entry (nnz no multiple of 4): the final partial chunk is read entry by entry."""
    c = case("ragged3001", np.dtype(dtype).name)
    nnz = len(c.col)
    assert nnz % 4 != 0
    h = {}
    for key, val in (("plain", c.val), ("special", c.val_special)):
        bufs = [synth.DeviceBuffer(a.nbytes) for a in (c.off, c.col, val)]
        for b, a in zip(bufs, (c.off, c.col, val)):
            b.upload(a)
        h[key] = sm.SparseMatCRS.from_device_parts(c.n_rows, c.n_cols, nnz, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, c.dtype.type, keep=tuple(bufs))
    sweep(c, h, "stream", "stream, borrowed arrays", exact=True)
    sweep(c, h, "vector", "vector, borrowed arrays")


@DTYPES
@pytest.mark.parametrize("where", ["first", "last"])
def test_merge_carry_takes_an_inf_along(gpu, dtype, where):
    """A row spanning several merge tiles whose only non-finite product lies in its first tile (it travels through the carry fix-up)
    or in its last; the rows around it stay what they were."""
    off, col, val, x = sp.merge_long_row(dtype, where)
    cls = sp.row_classes(off, col, val, x)
    assert cls[2] in (1, 2) and (np.delete(cls, 2) == 0).all()
    m = sm.SparseMatCRS.from_raw_parts(6, 10000, off, col, val)
    rows, nz, items = m.merge_table()
    assert m.resolved_variant()[0] == "merge" and len(rows) - 1 >= 3 and 9001 > 2 * items   # the row spans several tiles
    for v in ("merge", "vector", "auto"):
        y = m.mvp(x, variant=v)
        assert_spmv_close(y, off, col, val, x, "long row, Inf %s, %s" % (where, v))
        assert np.array_equal(value_class(y), cls) and not bits(y[[0, 1, 3, 5]]).any()
        assert np.array_equal(bits(y), bits(m.mvp(x, variant=v)))


# ---- K1r: one window, the wide ring, four bands; 16-bit column copy on and off ---------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["banded3000x7", "wide_band", "stencil_planes"])
def test_ring_forms(gpu, dtype, name):
    c = case(name, np.dtype(dtype).name)
    h = c.handles(lambda m: m.set_ring(1))
    for m in h.values():
        nb, frac, active, _, _ = m.ring_plan()
        if name == "banded3000x7":
            assert active and frac == 1.0 and m.ring_bands() == 1 and m.ring_entries() == 16384
        elif name == "wide_band" and dtype == np.float32:
            assert active and frac > 0.9 and m.ring_bands() == 1 and m.ring_entries() == 32768
        elif name == "wide_band":
            assert active and m.ring_entries() == 16384 and 0.1 < frac < 0.9  # f64 keeps the narrow ring: ring phases and global gathers
        else:
            assert active and frac > 0.9 and m.ring_bands() == 4
    for lanes in (2, 4, 8, 16):
        for m in h.values():
            m.set_vector_lanes(lanes)
        # (the banded plan streams the 16-bit column copy whatever the knob says: "0" changes nothing on stencil_planes)
        for col16 in ("1", "0"):
            with_env("SMH_RING_COL16", col16, lambda: sweep(c, h, "vector", "K1r lanes %d col16 %s" % (lanes, col16), inner_prod=(lanes == 8 and col16 == "1")))


# ---- K1s: coded (C16) / plain columns, XS, XD, XD-V -------------------------------------------------------------------------------
def stream_forms(c, h, want_chunks, dict_sizes):
    """Every body of the CSR-stream kernel on one matrix; dict_sizes: what the value dictionary may hold per value array."""
    for m in h.values():
        assert m.stream_layout()["xs_chunks"] == 0 and not m.stream_direct()   # x is small: not staged by default
    for c16 in ("1", "0"):
        with_env("SMH_STREAM_C16", c16, lambda: sweep(c, h, "stream", "K1s C16=%s" % c16, exact=True, inner_prod=(c16 == "1")))
    for m in h.values():
        assert m.stream_layout()["coded"]
        m.set_stream_xs(1)
        m.set_stream_direct(0)
        assert m.stream_layout()["xs_chunks"] == want_chunks and not m.stream_direct() and len(m.stream_value_dict()) == 0
    sweep(c, h, "stream", "K1s XS", exact=True, inner_prod=True)
    for m in h.values():
        m.set_stream_direct(1)
        m.set_stream_value_dict(0)
        assert m.stream_direct() and len(m.stream_value_dict()) == 0
    sweep(c, h, "stream", "K1s XD", exact=True, inner_prod=True)
    for key, m in h.items():
        m.set_stream_value_dict(-1)
        assert m.stream_direct() and len(m.stream_value_dict()) in dict_sizes[key], (key, len(m.stream_value_dict()))
    sweep(c, h, "stream", "K1s XD-V", exact=True, inner_prod=True)


@DTYPES
@pytest.mark.parametrize("name,chunks", [("stencil48", 2), ("stencil1000", 4), ("xd_long_rows", 2)])
def test_stream_forms(gpu, dtype, name, chunks):
    c = case(name, np.dtype(dtype).name)
    if name == "xd_long_rows":
        assert c.lens.max() == 40 and (c.lens == 23).any()
        sizes = {"plain": (0,), "special": (0,)}                             # arbitrary values: no dictionary
    else:
        # the stencil's two values; with val_special the five patterns +Inf, -Inf, NaN, +0.0, -0.0 beside them: the dictionary holds
        # them by their bits or declines -- both are right, the result decides
        sizes = {"plain": (2,), "special": (0, 7)}
    stream_forms(c, c.handles(), chunks, sizes)


@DTYPES
@pytest.mark.parametrize("n_values", [6, 20, 7])
@pytest.mark.parametrize("name", ["stencil48", "xd_long_rows"])
def test_value_dictionary_of_special_values(gpu, dtype, name, n_values):
    """K1s XD-V multiplies by a dictionary entry picked by code bits: both dictionary forms (<= 8 values, 9-32 values), a dictionary
    that holds +0.0, -0.0, +Inf and a NaN, rows beyond 8 entries; n_values 7: one value is the NaN pattern the dictionary's build
    uses for an empty slot (it declines such a matrix).  0 * Inf = NaN through the dictionary as through the value array."""
    c = case(name, np.dtype(dtype).name)
    u = np.uint32 if dtype == np.float32 else np.uint64
    rng = np.random.default_rng(n_values)
    pool = np.concatenate([np.array([0.0, -0.0, np.inf, np.nan], dtype), ((np.arange(n_values - 4) + 1) * 0.043 - 0.4).astype(dtype)])
    if n_values == 7:
        pool.view(u)[3] = 0x7FC5A5A5 if dtype == np.float32 else 0x7FF8A5A55A5AA5A5
    # mostly the ordinary values; each special a little under 1 % of the entries
    pick = np.where(rng.random(len(c.col)) < 0.03, rng.integers(0, 4, len(c.col)), rng.integers(4, n_values, len(c.col)))
    val = pool[pick]
    val[:n_values] = pool
    xs = c.inputs[0][2]
    for x in (xs, sp.x_finite(9, c.n_cols, dtype)):
        y_ref = oracle.spmv(c.off, c.col, val, x)
        cls = sp.row_classes(c.off, c.col, val, x)
        assert 0.05 < sp.finite_share(c.off, cls) < 0.95
        m = sm.SparseMatCRS.from_raw_parts(c.n_rows, c.n_cols, c.off, c.col, val)
        m.set_stream_xs(1)
        m.set_stream_direct(1)
        d = m.stream_value_dict()
        assert m.stream_direct() and len(d) in ((0,) if n_values == 7 else (0, n_values)), len(d)
        if len(d):
            assert np.array_equal(np.sort(bits(d)), np.sort(bits(pool)))
        ys = []
        for use_dict in (-1, 0):
            m.set_stream_value_dict(use_dict)
            y = m.mvp(x, variant="stream")
            check_y(c, y, "%d values" % n_values, val, x, y_ref, cls, "dictionary %d" % use_dict, exact=True)
            ys.append(y)
        assert same_bits(ys[0], ys[1])


# ---- K2c, K2f, K2s ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("shift,n_blocks", [(8, 20), (11, 3)])
def test_column_blocked_forms(gpu, dtype, shift, n_blocks):
    c = case("colblock6007", np.dtype(dtype).name)
    h = c.handles(lambda m: m.set_colblock_shift(shift))
    for m in h.values():
        assert m.colblock(arrays=False)["n_blocks"] == n_blocks and m.colfused(arrays=False)["fits"]
        assert m.colfused(arrays=False)["n_blocks"] == n_blocks
    sweep(c, h, "colblock", "K2c, %d blocks" % n_blocks)
    sweep(c, h, "colfused", "K2f, %d blocks" % n_blocks)


@DTYPES
def test_colsplit_form(gpu, dtype):
    c = case("colsplit9001", np.dtype(dtype).name)
    h = c.handles(lambda m: m.set_colblock_shift(9))
    for m in h.values():
        cs = m.colsplit()
        assert cs["split"] and cs["min_long"] == 64 and cs["n_long"] == int((c.lens >= 64).sum())
    sweep(c, h, "colsplit", "K2s")


# ---- K2t -------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["tiled_skewed", "tiled_rounds", "tiled_64chunks"])
def test_tiled_forms(gpu, dtype, name):
    c = case(name, np.dtype(dtype).name)
    h = c.handles()
    for m in h.values():
        lay = m.tiled_layout(arrays=True)
        per_slice = np.diff(lay["slice_chunks"].astype(np.int64))
        tiles = np.diff(lay["tile_start"].astype(np.int64), axis=0)
        if name == "tiled_skewed":      # 5 slices, the last short; (row, slice) pairs cut by a chunk boundary: more runs than pairs
            ch = lay["copy_entries"] // len(lay["chunks"])
            have = np.arange(ch)[None, :] < lay["chunks"][:, 1].astype(np.int64)[:, None]
            runs = int((have & ((lay["codes"].reshape(-1, ch) & 0x8000) == 0)).sum())
            rows = np.repeat(np.arange(c.n_rows), c.lens)
            pairs = len(np.unique(rows * 5 + c.col // sp.SLICE))
            assert lay["n_slices"] == 5 and c.n_cols % sp.SLICE != 0 and runs >= pairs + 5, (runs, pairs)
        elif name == "tiled_rounds":    # every product in the first slice's tiles: several rounds of 64 lanes x 16 bytes
            assert lay["n_slices"] == 4 and tiles[:, 0].max() > (256 if dtype == np.float32 else 128) and not tiles[:, 1:].any()
        else:                           # one part of 64 chunks per wavefront
            assert lay["n_slices"] == 16 and per_slice.max() == per_slice.sum() and (per_slice.max() + 15) // 16 == 64
    sweep(c, h, "tiled", "K2t")


# ---- the partitioned product ------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("n_blocks", [3, 4])
def test_partitioned_product(gpu, dtype, n_blocks):
    """Blocks on one device, overlap on / off, all-gather and window exchange, K1s and K1r per block; x_single's +Inf column once in
    a halo (other blocks reference it: it must arrive) and once in a block's interior (nobody else may see it)."""
    c = case("par_banded", np.dtype(dtype).name)
    n, r = c.n_rows, c.n_rows // n_blocks
    runs = [(tag, val, x, y_ref, cls) for tag, val, x, y_ref, cls in c.inputs if tag != "x_single"]
    for where, inf_col in (("halo", r + 3), ("interior", r + r // 2)):
        x, _ = sp.x_single(7, c.off, c.col, n, dtype, inf_col=inf_col)
        x = x[:n].copy()
        cls = sp.row_classes(c.off, c.col, c.val, x)
        hit_blocks = set((np.nonzero(cls)[0] // r).clip(0, n_blocks - 1).tolist())
        assert hit_blocks == ({0, 1} if where == "halo" else {1}), (where, hit_blocks)
        runs.append(("x_single " + where, c.val, x, oracle.spmv(c.off, c.col, c.val, x), cls))
    mats = {}
    for key, val in (("plain", c.val), ("special", c.val_special)):
        m = sm.SparseMatParLocal.with_sub_matrices(n_blocks, n, n, c.off, c.col, val, device_ids=[0] * n_blocks)
        assert m.exchange_mode("auto")[0] == "window"
        assert all(m.interior(b, v)[1] > m.interior(b, v)[0] for b in range(n_blocks) for v in ("stream", "vector"))
        mats[key] = m
    for tag, val, x, y_ref, cls in runs:
        m = mats["special" if tag.startswith("val_special") else "plain"]
        for variant in ("stream", "vector"):
            got = {}
            for overlap in (True, False):
                m.set_overlap(overlap)
                for exch in ("window", "allgather"):
                    xv, yv = m.vec(host=x), m.vec()
                    m.mvp_dev(xv, yv, variant=variant, exchange=exch)
                    m.synchronize()
                    y = yv.download()
                    check_y(c, y, tag, val, x, y_ref, cls, "%d blocks %s overlap %d %s" % (n_blocks, variant, overlap, exch), exact=(variant == "stream"))
                    got[(overlap, exch)] = y.tobytes()
            assert len(set(got.values())) == 1, (tag, variant)
        m.set_overlap(True)


# ---- gradual underflow -----------------------------------------------------------------------------------------------------------------
def underflow_forms(name, m):
    """(what, variant, exact, set-up) for every form a matrix of the underflow test goes through."""
    def lanes_ring(lanes, ring):
        def f():
            m.set_vector_lanes(lanes)
            m.set_ring(ring)
            assert m.ring_plan()[2] == bool(ring)
        return f

    def stream(xs, direct, use_dict):
        def f():
            m.set_stream_xs(xs)
            m.set_stream_direct(direct)
            m.set_stream_value_dict(use_dict)
            assert m.stream_direct() == bool(direct == 1) and (len(m.stream_value_dict()) > 0) == (use_dict == -1 and direct == 1)
        return f

    def shift(s, fused=False, split=False):
        def f():
            m.set_colblock_shift(s)
            assert m.colblock(arrays=False)["n_blocks"] >= 3 and (not fused or m.colfused(arrays=False)["fits"]) and (not split or m.colsplit()["split"])
        return f

    def tiled(n_slices):
        def f():
            assert m.tiled_layout()["n_slices"] == n_slices
        return f

    forms = [("seq", "seq", True, None), ("stream", "stream", True, None), ("merge", "merge", False, None), ("auto", "auto", False, None)]
    if name == "ragged3001":
        forms += [("vector lanes %d ring %d" % (l, r), "vector", False, lanes_ring(l, r)) for l in (1, 4, 8, 64) for r in (1, 0)]
        forms += [("K2c", "colblock", False, shift(8)), ("K2t", "tiled", False, tiled(1))]
    elif name == "stencil48":
        forms += [("K1s XS", "stream", True, stream(1, 0, 0)), ("K1s XD", "stream", True, stream(1, 1, 0)), ("K1s XD-V", "stream", True, stream(1, 1, -1)),
                  ("vector lanes 4", "vector", False, lanes_ring(4, 1))]
    elif name == "banded3000x7":
        forms += [("K1r lanes %d" % l, "vector", False, lanes_ring(l, 1)) for l in (2, 4, 8, 16)]
    elif name == "tiled_skewed":
        forms += [("K2t", "tiled", False, tiled(5)), ("K2c", "colblock", False, shift(12)), ("vector lanes 8", "vector", False, lanes_ring(8, 0))]
    elif name == "colblock6007":
        forms += [("K2c", "colblock", False, shift(8)), ("K2f", "colfused", False, shift(8, fused=True)), ("K2f 3 blocks", "colfused", False, shift(11, fused=True))]
    else:
        forms += [("K2s", "colsplit", False, shift(9, split=True))]
    return forms


@DTYPES
@pytest.mark.parametrize("positive", [False, True], ids=["signed", "positive"])
@pytest.mark.parametrize("name", sp.UNDERFLOW_MATRICES)
def test_gradual_underflow(gpu, dtype, name, positive):
    """Every product subnormal, the row sums around the smallest normal number.  SEQ and the K1s family: the oracle's bits.  Every
    other form, per row of length L: |y - exact| <= L q + 2 L eps sum|a x| (q the subnormal spacing) -- derived in
    special_model.underflow_bound, not measured; the oracle uses at most half of it, a result flushed to zero exceeds it many times.
    assert_spmv_close cannot see any of this: its '+ tiny' term covers the whole subnormal range."""
    n_rows, n_cols, off, col, val, x = sp.underflow_inputs(name, dtype, positive)
    exact, bound = sp.underflow_bound(off, col, val, x)
    y_ref = oracle.spmv(off, col, val, x)
    m = sm.SparseMatCRS.from_raw_parts(n_rows, n_cols, off, col, val)
    for what, variant, exact_bits, setup in underflow_forms(name, m):
        if setup is not None:
            setup()
        y = m.mvp(x, variant=variant)
        ratio = sp.underflow_ratio(y, exact, bound)
        print("underflow ratio %s %s %s %s: %.3f" % (name, np.dtype(dtype).name, "positive" if positive else "signed", what, ratio))
        assert ratio <= 1.0, (what, ratio)
        if exact_bits:
            assert np.array_equal(bits(y), bits(y_ref)), what
