"""SparseMatCRS: host-side mirror of the reference's ``SparseMatCRS<T,u32>`` (sparsemat_crs.rs) for
the SpMV hot path, backed by a device-resident ``smh_crs``.

The host owns the CRS arrays (``offset_rows``, ``columns``, ``values``); ``from_raw_parts`` copies
them to HBM once.  ``mvp`` / ``*`` run the hand-written HIP kernels.  Element access runs on the device too:
``get`` / ``get_many`` (SparseMatrix::get) and ``set`` / ``add_to`` / ``apply`` (a whole stream of set / add_to calls at
once, bit for bit the reference's get_mut placement and folds, see ``smh_crs_apply`` in the header).  One call per
operation is correct but slow: batch the stream into one ``apply``.
"""
import ctypes as C
import numbers

import numpy as np

from . import _lib
from ._lib import check, lib
from .densevec import DenseVec
from .multivec import MultiVec, pack_host


def _index(i):
    """A row or column index of Index = u32: larger (or negative) ones are refused, never truncated."""
    i = int(i)
    if not 0 <= i <= 0xFFFFFFFF:
        raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "index %d does not fit the u32 index type" % i)
    return i


class EigshResult:
    """What ``SparseMatCRS.eigsh`` returns."""
    __slots__ = ("values", "vectors", "estimates", "n_conv", "restarts", "products", "breakdown")

    def __init__(self, values, vectors, estimates, n_conv, restarts, products, breakdown):
        self.values, self.vectors, self.estimates = values, vectors, estimates
        self.n_conv, self.restarts, self.products, self.breakdown = n_conv, restarts, products, breakdown


class SparseMatCRS:
    def __init__(self, handle, dtype, keep=None):
        self._h = handle
        self._dtype = np.dtype(dtype)
        self._keep = keep

    # ---- constructors ------------------------------------------------------------------------
    @classmethod
    def from_raw_parts(cls, n_rows, n_cols, offset_rows, columns, values, validate=True):
        """Fills the gap the reference leaves (its only bulk constructor, from_sparsemat_index
        sparsemat_crs.rs:24-50, is pub(crate)): adopt CRS arrays as they are -- rows in storage
        order, unsorted, duplicates allowed."""
        values = np.ascontiguousarray(values)
        if values.dtype not in (np.float32, np.float64):
            raise TypeError("the HIP path handles f32/f64 values only (got %s)" % values.dtype)
        off = np.ascontiguousarray(offset_rows, dtype=np.uint32)
        col = np.ascontiguousarray(columns, dtype=np.uint32)
        if n_rows and len(off) != n_rows + 1:
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "offset_rows must have n_rows+1 entries")
        if len(col) != len(values):
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "columns and values differ in length")
        h = C.c_void_p()
        check(lib().smh_crs_create(_lib.dtype_code(values.dtype), n_rows, n_cols, len(values),
                                   off.ctypes.data if len(off) else None,
                                   col.ctypes.data if len(col) else None,
                                   values.ctypes.data if len(values) else None,
                                   1 if validate else 0, C.byref(h)))
        return cls(h, values.dtype)

    @classmethod
    def from_device_parts(cls, n_rows, n_cols, nnz, off_ptr, col_ptr, val_ptr, dtype, keep=None,
                          validate=False):
        """Borrow CRS arrays already resident in HBM (raw device pointers); ``keep`` is held alive."""
        h = C.c_void_p()
        check(lib().smh_crs_create_dev(_lib.dtype_code(dtype), n_rows, n_cols, nnz, C.c_void_p(off_ptr),
                                       C.c_void_p(col_ptr), C.c_void_p(val_ptr), 1 if validate else 0,
                                       C.byref(h)))
        return cls(h, dtype, keep)

    @classmethod
    def from_triplets(cls, rows, cols, values, ops=None, into_crs=False):
        """The CRS the reference ends up with after the call stream ``mat.add_to(rows[k], cols[k], values[k])``
        (``ops[k] == 1``: ``mat.set(...)``) on a SparseMatIndexList and ``to_crs()``
        (sparsemat_indexlist.rs:61-63,158-164; sparsemat_crs.rs:24-50) -- built on the device, bit-exact:
        entries of a row in order of first appearance, duplicates folded in stream order.
        ``into_crs=True``: the stream is applied to a SparseMatCRS itself (sparsemat_crs.rs:54-92,143-149): rows in
        reverse order of first appearance, first-push quirk included (see ``smh_crs_replay`` in the header)."""
        values = np.ascontiguousarray(values)
        if values.dtype not in (np.float32, np.float64):
            raise TypeError("the HIP path handles f32/f64 values only (got %s)" % values.dtype)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        n = len(values)
        if len(rows) != n or len(cols) != n:
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "rows, cols and values differ in length")
        ops_a = None if ops is None else np.ascontiguousarray(ops, dtype=np.uint8)
        if ops_a is not None and len(ops_a) != n:
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "ops and values differ in length")
        h = C.c_void_p()
        fn = lib().smh_crs_replay if into_crs else lib().smh_crs_assemble
        check(fn(_lib.dtype_code(values.dtype), n, rows.ctypes.data if n else None, cols.ctypes.data if n else None,
                 values.ctypes.data if n else None, ops_a.ctypes.data if (ops_a is not None and n) else None, C.byref(h)))
        return cls(h, values.dtype)

    @classmethod
    def from_device_triplets(cls, n_ops, rows_ptr, cols_ptr, vals_ptr, dtype, ops_ptr=None, into_crs=False):
        """``from_triplets`` over operation arrays that already live in HBM (raw device pointers)."""
        h = C.c_void_p()
        fn = lib().smh_crs_replay_dev if into_crs else lib().smh_crs_assemble_dev
        check(fn(_lib.dtype_code(dtype), n_ops, C.c_void_p(rows_ptr), C.c_void_p(cols_ptr), C.c_void_p(vals_ptr),
                 C.c_void_p(ops_ptr or 0), C.byref(h)))
        return cls(h, dtype)

    @classmethod
    def new(cls, dtype=np.float32):
        """SparseMatCRS::new() (sparsemat_crs.rs:47-49): no rows, no entries."""
        h = C.c_void_p()
        check(lib().smh_crs_replay(_lib.dtype_code(np.dtype(dtype)), 0, None, None, None, None, C.byref(h)))
        return cls(h, dtype)

    @classmethod
    def eye(cls, dim, dtype=np.float32):
        """SparseMatrix::eye (sparsematrix.rs:91-98) on a SparseMatCRS: ``set(i, i, 1)`` for i < dim.  dim 1 keeps the
        container's first-push quirk (no rows, one orphan); dim >= 2 is the identity."""
        h = C.c_void_p()
        check(lib().smh_crs_eye(_lib.dtype_code(np.dtype(dtype)), int(dim), C.byref(h)))
        return cls(h, dtype)

    def transpose(self):
        """SparseMatrix::transpose (sparsematrix.rs:174-184): ``ret.set(j, i, val)`` for every entry in row-major
        storage order into a fresh SparseMatCRS -- on the device, bit-exact including the storage order the
        reference's CRS container produces (rows reversed, first-push quirk)."""
        h = C.c_void_p()
        check(lib().smh_crs_transpose(self._h, C.byref(h)))
        return type(self)(h, self.dtype)

    @staticmethod
    def last_transpose_route():
        """"general" (stable sort by target row) or "bucketed" (two bucketed passes, csrc/transpose_bucket.hip): how this
        thread's last ``transpose`` was carried out."""
        return ("general", "bucketed")[lib().smh_last_transpose_route()]

    def column_info(self):
        """ColumnIter::assemble_column_info (sparsemat_crs.rs:180-191) as arrays ``(rows, col_ptr, entries)``:
        ``rows[k]`` = row of entry k; column j's entries in storage order are ``entries[col_ptr[j]:col_ptr[j+1]]``."""
        nnz, n_cols = self.n_non_zero_entries(), self.n_cols()
        rows = np.zeros(max(nnz, 1), np.uint32)
        col_ptr = np.zeros(n_cols + 1, np.uint32)
        entries = np.zeros(max(nnz, 1), np.uint32)
        check(lib().smh_crs_column_info(self._h, rows.ctypes.data, col_ptr.ctypes.data, entries.ctypes.data))
        return rows[:nnz], col_ptr, entries[:nnz]

    def iter_col(self, col, info=None, values=None):
        """ColumnIter::iter_col (sparsemat_crs.rs:193-204): the (row, value) pairs of a column in storage order.
        ``info`` = a ``column_info()`` result and ``values`` the downloaded values, to avoid repeating both."""
        rows, col_ptr, entries = info if info is not None else self.column_info()
        if values is None:
            values = self.raw_parts()[2]
        e = entries[col_ptr[col]:col_ptr[col + 1]] if col < len(col_ptr) - 1 else entries[:0]
        return list(zip(rows[e].tolist(), values[e].tolist()))

    def prod(self, rhs):
        """SparseMatrix::prod (sparsematrix.rs:186-210): the SparseMatCRS the reference's loops build for
        ``self.prod(&rhs)`` -- same sums (order of additions included), zero sums dropped, rows in descending column
        order.  Err("Dimension mismatch") becomes a SparseMatPanic with that text."""
        h = C.c_void_p()
        check(lib().smh_crs_prod(self._h, rhs._h, C.byref(h)))
        return type(self)(h, self.dtype)

    # ---- reordering (an extension: the reference has none; csrc/permute.hip, csrc/reorder.hip) ---------------------------
    @staticmethod
    def _perm_arg(perm):
        if perm is None:
            return None, None, 0
        a = np.ascontiguousarray(perm, dtype=np.uint32)
        keep = a if len(a) else np.zeros(1, np.uint32)  # (a pointer even for an empty array: NULL means the identity)
        return keep, keep.ctypes.data, len(a)

    def permute(self, row_perm=None, col_perm=None):
        """``out[i][j] = self[row_perm[i]][col_perm[j]]`` as a new matrix (``perm[new] = old``, scipy's ``A[perm][:, perm]``): rows
        keep their entries in storage order, columns are relabelled, values are copied bit for bit.  None = identity."""
        rk, rp, rn = self._perm_arg(row_perm)
        ck, cp, cn = self._perm_arg(col_perm)
        h = C.c_void_p()
        check(lib().smh_crs_permute(self._h, rp, rn, cp, cn, C.byref(h)))
        return type(self)(h, self.dtype)

    def permute_symmetric(self, perm):
        """``P A P^T``: ``permute(perm, perm)`` of a square matrix."""
        keep, p, n = self._perm_arg(perm if perm is not None else [])
        h = C.c_void_p()
        check(lib().smh_crs_permute_symmetric(self._h, p, n, C.byref(h)))
        return type(self)(h, self.dtype)

    def rcm(self):
        """The reverse Cuthill-McKee ordering of the (symmetrised) pattern, computed on the device: ``(perm, stats)`` with
        ``perm`` an ``np.uint32`` array ready for ``permute_symmetric`` and ``stats = dict(n_components, n_levels)``.  One
        round of kernels per level: a chain of n vertices takes n rounds."""
        n = self.n_rows()
        perm = np.zeros(max(n, 1), np.uint32)
        comps, levels = C.c_size_t(), C.c_size_t()
        check(lib().smh_crs_rcm(self._h, perm.ctypes.data, C.byref(comps), C.byref(levels)))
        return perm[:n], dict(n_components=comps.value, n_levels=levels.value)

    def color(self, seed=0):
        """A multicolour ordering of the (symmetrised) pattern, computed on the device (``smh_crs_color``: greedy in the order of
        the keys ``deg << 32 | mix(v ^ seed)``, largest first): ``(perm, stats)`` with ``perm`` an ``np.uint32`` array ready for
        ``permute_symmetric`` -- the rows sorted by (colour, index) -- and ``stats = dict(colors (np.uint32, by ORIGINAL row),
        n_colors, n_rounds, color_counts)``.  The triangular solves of the permuted matrix have at most ``n_colors`` levels."""
        n = self.n_rows()
        perm = np.zeros(max(n, 1), np.uint32)
        colors = np.zeros(max(n, 1), np.uint32)
        n_colors, n_rounds = C.c_size_t(), C.c_size_t()
        check(lib().smh_crs_color(self._h, int(seed) & 0xFFFFFFFF, colors.ctypes.data, perm.ctypes.data, C.byref(n_colors), C.byref(n_rounds)))
        colors = colors[:n]
        return perm[:n], dict(colors=colors, n_colors=n_colors.value, n_rounds=n_rounds.value,
                              color_counts=np.bincount(colors, minlength=n_colors.value))

    # ---- sparse triangular solves and symmetric Gauss-Seidel (extensions; csrc/trisolve.hip, csrc/pcg.hip) ------------------
    def trisolve_levels(self, uplo="lower"):
        """The level schedule of the ``uplo`` triangle (``smh_crs_trisolve_levels``; built on the device on first use):
        dict(n_levels, level_of_row (np.uint32, n_rows), n_launches -- kernel launches one solve enqueues --, small_level_rows --
        the R up to which consecutive levels share one single-workgroup launch)."""
        n = self.n_rows()
        lev = np.zeros(max(n, 1), np.uint32)
        n_levels, n_launches, small = C.c_size_t(), C.c_size_t(), C.c_size_t()
        check(lib().smh_crs_trisolve_levels(self._h, _lib.UPLO[uplo], C.byref(n_levels), lev.ctypes.data, C.byref(n_launches), C.byref(small)))
        return dict(n_levels=n_levels.value, level_of_row=lev[:n], n_launches=n_launches.value, small_level_rows=small.value)

    def trisolve(self, b, uplo="lower", unit_diagonal=False):
        """x = T^-1 b with T the ``uplo`` triangle of this square matrix (the first stored (i, i) of a row is its diagonal entry;
        ``unit_diagonal``: an implied 1): level-scheduled on the device, every operation rounded once, the subtractions of a row
        in storage order (``smh_crs_trisolve*``).  A ``DenseVec`` b gives a new ``DenseVec``; anything else a numpy array."""
        diag = _lib.SMH_DIAG_UNIT if unit_diagonal else _lib.SMH_DIAG_NON_UNIT
        if isinstance(b, DenseVec):
            x = DenseVec.zeros(b.dim(), self.dtype)
            check(lib().smh_crs_trisolve_vec(self._h, _lib.UPLO[uplo], diag, b._h, x._h))
            return x
        bb = np.ascontiguousarray(b, dtype=self.dtype)
        x = np.zeros(bb.size, self.dtype)
        check(lib().smh_crs_trisolve(self._h, _lib.UPLO[uplo], diag, bb.ctypes.data if bb.size else None, bb.size,
                                     x.ctypes.data if x.size else None, x.size))
        return x

    def sgs_apply(self, r):
        """z = M^-1 r with the symmetric Gauss-Seidel preconditioner M = (D + L) D^-1 (D + U) of this matrix
        (``smh_crs_sgs_apply_vec``).  A ``DenseVec`` r gives a new ``DenseVec``; anything else a numpy array."""
        if isinstance(r, DenseVec):
            z = DenseVec.zeros(r.dim(), self.dtype)
            check(lib().smh_crs_sgs_apply_vec(self._h, r._h, z._h))
            return z
        rv = DenseVec.from_vec(np.ascontiguousarray(r, dtype=self.dtype))
        z = DenseVec.zeros(rv.dim(), self.dtype)
        check(lib().smh_crs_sgs_apply_vec(self._h, rv._h, z._h))
        return z.to_numpy()

    # ---- ILU(0) (an extension; csrc/ilu.hip, applied through csrc/pcg.hip) ------------------------------------------------
    _NO_PIVOT = C.c_size_t(-1).value  # SIZE_MAX: no zero pivot

    def ilu0(self):
        """``(f, zero_pivot)``: the incomplete LU factorization without fill of this square matrix (``smh_crs_ilu0``), factored
        on the device level by level of the lower schedule.  ``f`` is a new matrix on this one's pattern whose values are the
        unit-lower L below the diagonal and U on and above it; ``zero_pivot`` is None, or the first row whose U(i, i) is 0 (not
        an error: the values are IEEE's).  Every row must be strictly ascending (``sort_rows``) and store its diagonal."""
        h, zp = C.c_void_p(), C.c_size_t()
        check(lib().smh_crs_ilu0(self._h, C.byref(h), C.byref(zp)))
        return type(self)(h, self.dtype), (None if zp.value == self._NO_PIVOT else zp.value)

    def ilu0_refactor(self, a):
        """This factor again from the values of ``a``, which has the pattern this factor was made on (``smh_crs_ilu0_refactor``):
        the bits of ``a.ilu0()`` without a new handle or schedule.  Returns ``zero_pivot`` as ``ilu0`` does."""
        zp = C.c_size_t()
        check(lib().smh_crs_ilu0_refactor(self._h, a._h, C.byref(zp)))
        return None if zp.value == self._NO_PIVOT else zp.value

    def ilu_apply(self, r):
        """z = U^-1 L^-1 r with this matrix an ``ilu0`` factor: a unit-lower and an upper triangular solve
        (``smh_crs_ilu_apply_vec``).  A ``DenseVec`` r gives a new ``DenseVec``; anything else a numpy array."""
        if isinstance(r, DenseVec):
            z = DenseVec.zeros(r.dim(), self.dtype)
            check(lib().smh_crs_ilu_apply_vec(self._h, r._h, z._h))
            return z
        rv = DenseVec.from_vec(np.ascontiguousarray(r, dtype=self.dtype))
        z = DenseVec.zeros(rv.dim(), self.dtype)
        check(lib().smh_crs_ilu_apply_vec(self._h, rv._h, z._h))
        return z.to_numpy()

    # ---- FSAI (an extension; csrc/fsai.hip, applied through csrc/pcg.hip) --------------------------------------------------
    def fsai(self):
        """``(g, gt, not_spd)``: the factorized sparse approximate inverse of this square matrix on the pattern of its lower
        triangle (``smh_crs_fsai``), one data-parallel sweep on the device.  ``g`` is lower triangular with G^T G ~ A^-1 and
        diag(G A G^T) = 1 for an SPD matrix, ``gt`` its transpose -- two ordinary matrices; z = G^T (G r) is two products
        (``g.fsai_apply(gt, r)``).  ``not_spd`` is None, or the first row whose last pivot is not > 0 (not an error: the values
        are IEEE's).  Every row must be strictly ascending (``sort_rows``), store its diagonal, and hold at most 128 entries on
        or below it; only those entries are read."""
        g, gt, bad = C.c_void_p(), C.c_void_p(), C.c_size_t()
        check(lib().smh_crs_fsai(self._h, C.byref(g), C.byref(gt), C.byref(bad)))
        return type(self)(g, self.dtype), type(self)(gt, self.dtype), (None if bad.value == self._NO_PIVOT else bad.value)

    def fsai_apply(self, gt, r, out=None):
        """z = G^T (G r) with this matrix the ``g`` and ``gt`` the transpose of ``fsai`` (``smh_crs_fsai_apply_vec``): two products.
        A ``DenseVec`` r gives a new ``DenseVec``, or ``out`` (which may be r itself); anything else a numpy array."""
        if isinstance(r, DenseVec):
            z = DenseVec.zeros(r.dim(), self.dtype) if out is None else out
            check(lib().smh_crs_fsai_apply_vec(self._h, gt._h, r._h, z._h))
            return z
        rv = DenseVec.from_vec(np.ascontiguousarray(r, dtype=self.dtype))
        z = DenseVec.zeros(rv.dim(), self.dtype)
        check(lib().smh_crs_fsai_apply_vec(self._h, gt._h, rv._h, z._h))
        return z.to_numpy()

    def fsai_ns(self):
        """``(gl, gu, singular)``: the non-symmetric factorized sparse approximate inverse of this square matrix
        (``smh_crs_fsai_ns``), G_U G_L ~ A^-1 -- two ordinary matrices.  ``gl`` is lower triangular on the stored (i, c) with c <= i,
        unit diagonal, G_L ~ L^-1 of A = L D U; ``gu`` is upper triangular on the stored (i, c) with c >= i; z = G_U (G_L r) is two
        products (``gl.fsai_ns_apply(gu, r)``).  On a dense pattern G_U G_L = A^-1.  ``singular`` is None, or the first row whose
        last pivot, in either factor's row solve, is zero or not finite (not an error: the values are IEEE's).  Every row must be
        strictly ascending (``sort_rows``) and store its diagonal; a row may hold at most 128 entries on or below it and a column
        at most 128 on or above it."""
        gl, gu, bad = C.c_void_p(), C.c_void_p(), C.c_size_t()
        check(lib().smh_crs_fsai_ns(self._h, C.byref(gl), C.byref(gu), C.byref(bad)))
        return type(self)(gl, self.dtype), type(self)(gu, self.dtype), (None if bad.value == self._NO_PIVOT else bad.value)

    def fsai_ns_apply(self, gu, r, out=None):
        """z = G_U (G_L r) with this matrix the ``gl`` and ``gu`` the other factor of ``fsai_ns`` (``smh_crs_fsai_ns_apply_vec``):
        ``fsai_apply`` under the name of the non-symmetric pair."""
        if isinstance(r, DenseVec):
            z = DenseVec.zeros(r.dim(), self.dtype) if out is None else out
            check(lib().smh_crs_fsai_ns_apply_vec(self._h, gu._h, r._h, z._h))
            return z
        rv = DenseVec.from_vec(np.ascontiguousarray(r, dtype=self.dtype))
        z = DenseVec.zeros(rv.dim(), self.dtype)
        check(lib().smh_crs_fsai_ns_apply_vec(self._h, gu._h, rv._h, z._h))
        return z.to_numpy()

    def bandwidth(self):
        """(max i - j, max j - i) over the stored entries; (0, 0) without entries."""
        lo, hi = C.c_uint32(), C.c_uint32()
        check(lib().smh_crs_bandwidth(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def span_fraction(self):
        """Mean column span of a 64-row tile / n_cols: the locality statistic AUTO tests."""
        out = C.c_double()
        check(lib().smh_crs_span_fraction(self._h, C.byref(out)))
        return out.value

    def clone(self):
        """#[derive(Clone)] (sparsemat_crs.rs:8): an independent library-owned copy (dims, arrays, orphans, kernel settings)."""
        h = C.c_void_p()
        check(lib().smh_crs_clone(self._h, C.byref(h)))
        return type(self)(h, self.dtype)

    def astype(self, dtype):
        """A new library-owned matrix of ``dtype`` (f32 or f64) with this one's dims, pattern, orphan and kernel settings, its
        values converted on the device (``smh_crs_cast``, an extension): f64 -> f32 rounds to nearest even, f32 -> f64 is exact; the
        same dtype gives ``clone()``.  The result's ``overflow`` is the number of finite values that became infinite."""
        h, over = C.c_void_p(), C.c_size_t()
        check(lib().smh_crs_cast(self._h, _lib.dtype_code(dtype), C.byref(h), C.byref(over)))
        out = type(self)(h, dtype)
        out.overflow = over.value
        return out

    def add(self, rhs):
        """SparseMatrix::add (sparsematrix.rs:123-133), in place like the reference's ``&mut self``: ``*get_mut(i, j) += val``
        for every entry of ``rhs`` in storage order -- new columns pushed to the start of their row, folds into the first
        occurrence; bit for bit (``smh_crs_add_assign``).  ``rhs`` may be ``self``."""
        check(lib().smh_crs_add_assign(self._h, rhs._h))

    def sub(self, rhs):
        """SparseMatrix::sub (sparsematrix.rs:135-143): as ``add`` with ``-=``."""
        check(lib().smh_crs_sub_assign(self._h, rhs._h))

    def __iadd__(self, rhs):  # AddAssign (sparsematrix.rs:372-378)
        if not isinstance(rhs, SparseMatCRS):
            return NotImplemented
        self.add(rhs)
        return self

    def __isub__(self, rhs):  # SubAssign (:380-386)
        if not isinstance(rhs, SparseMatCRS):
            return NotImplemented
        self.sub(rhs)
        return self

    def __add__(self, rhs):  # Add: self.clone() += rhs (:397-407)
        if not isinstance(rhs, SparseMatCRS):
            return NotImplemented
        h = C.c_void_p()
        check(lib().smh_crs_add(self._h, rhs._h, C.byref(h)))
        return type(self)(h, self.dtype)

    def __sub__(self, rhs):  # Sub: self.clone() -= rhs (:409-419)
        if not isinstance(rhs, SparseMatCRS):
            return NotImplemented
        h = C.c_void_p()
        check(lib().smh_crs_sub(self._h, rhs._h, C.byref(h)))
        return type(self)(h, self.dtype)

    @staticmethod
    def last_add_route():
        """How this thread's last add / sub was carried out (``smh_last_add_route``): "general", "short_rows",
        "structure_unchanged" or "same_pattern"."""
        return ("general", "short_rows", "structure_unchanged", "same_pattern")[lib().smh_last_add_route()]

    # ---- element access (sparsematrix.rs:224-233, sparsemat_crs.rs:54-92, 136-150) ----------------
    def get(self, i, j):
        """SparseMatrix::get: the first entry of row i with column j, zero when absent or i >= n_rows."""
        out = np.zeros(1, self._dtype)
        check(lib().smh_crs_get(self._h, int(i), int(j), out.ctypes.data))
        return out[0]

    def get_many(self, rows, cols):
        """``get`` for every (rows[k], cols[k]) at once -> numpy array of the value type."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        if len(rows) != len(cols):
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "rows and cols differ in length")
        n = len(rows)
        out = np.zeros(n, self._dtype)
        check(lib().smh_crs_get_many(self._h, n, rows.ctypes.data if n else None, cols.ctypes.data if n else None,
                                     out.ctypes.data if n else None))
        return out

    def get_many_dev(self, n, rows_ptr, cols_ptr, out_ptr):
        """``get_many`` on raw device pointers (u32 rows / cols, values of the handle's dtype)."""
        check(lib().smh_crs_get_many_dev(self._h, int(n), C.c_void_p(rows_ptr), C.c_void_p(cols_ptr), C.c_void_p(out_ptr)))

    def apply(self, rows, cols, values, ops=None):
        """``add_to(rows[k], cols[k], values[k])`` (``ops[k] == 1``: ``set``) for every k in stream order, in place, bit for
        bit (``smh_crs_apply``).  Re-assembly into the handle's own pattern updates the values where they are.  A float array
        of the other value type is refused (no silent rounding)."""
        values = np.asarray(values)
        if values.dtype.kind == "f" and values.dtype != self._dtype:
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "values are %s, the matrix holds %s" % (values.dtype, self._dtype))
        values = np.ascontiguousarray(values, dtype=self._dtype)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        n = len(values)
        if len(rows) != n or len(cols) != n:
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "rows, cols and values differ in length")
        ops_a = None if ops is None else np.ascontiguousarray(ops, dtype=np.uint8)
        if ops_a is not None and len(ops_a) != n:
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "ops and values differ in length")
        check(lib().smh_crs_apply(self._h, n, rows.ctypes.data if n else None, cols.ctypes.data if n else None,
                                  values.ctypes.data if n else None, ops_a.ctypes.data if (ops_a is not None and n) else None))

    def apply_dev(self, n_ops, rows_ptr, cols_ptr, vals_ptr, ops_ptr=None):
        """``apply`` over operation arrays that already live in HBM (raw device pointers; ``ops_ptr`` may be None)."""
        check(lib().smh_crs_apply_dev(self._h, int(n_ops), C.c_void_p(rows_ptr), C.c_void_p(cols_ptr), C.c_void_p(vals_ptr),
                                      C.c_void_p(ops_ptr or 0)))

    def update_plan(self, rows, cols, ops=None):
        """A reusable plan for re-assembling this matrix from the stream ``(rows[k], cols[k], ops[k])`` with new values
        (``smh_update_plan_create``): every operation must land on an existing entry -- ``apply`` the stream once to create
        them, then plan.  Valid until the structure changes (``sort_rows``, an ``apply`` / ``+=`` that adds entries)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        n = len(rows)
        if len(cols) != n:
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "rows and cols differ in length")
        ops_a = None if ops is None else np.ascontiguousarray(ops, dtype=np.uint8)
        if ops_a is not None and len(ops_a) != n:
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "ops and rows differ in length")
        h = C.c_void_p()
        check(lib().smh_update_plan_create(self._h, n, rows.ctypes.data if n else None, cols.ctypes.data if n else None,
                                           ops_a.ctypes.data if (ops_a is not None and n) else None, C.byref(h)))
        return UpdatePlan(h, self, n)

    def update_plan_dev(self, n_ops, rows_ptr, cols_ptr, ops_ptr=None):
        """``update_plan`` over operation arrays that already live in HBM (raw device pointers; ``ops_ptr`` may be None)."""
        h = C.c_void_p()
        check(lib().smh_update_plan_create_dev(self._h, int(n_ops), C.c_void_p(rows_ptr), C.c_void_p(cols_ptr), C.c_void_p(ops_ptr or 0),
                                               C.byref(h)))
        return UpdatePlan(h, self, int(n_ops))

    def set(self, i, j, value):
        """SparseMatrix::set (sparsematrix.rs:226-228): one ``apply`` -- correct, but a device round trip per call."""
        self.apply([_index(i)], [_index(j)], np.array([value], self._dtype), [1])

    def add_to(self, i, j, value):
        """SparseMatrix::add_to (sparsematrix.rs:231-233): one ``apply`` -- correct, but a device round trip per call."""
        self.apply([_index(i)], [_index(j)], np.array([value], self._dtype))

    @staticmethod
    def last_apply_route():
        """How this thread's last ``apply`` was carried out (``smh_last_apply_route``): "general", "values_only" or
        "replay"."""
        return ("general", "values_only", "replay")[lib().smh_last_apply_route()]

    def is_symmetric(self):  # sparsematrix.rs:212-222
        out = C.c_int(0)
        check(lib().smh_crs_is_symmetric(self._h, C.byref(out)))
        return bool(out.value)

    def is_sorted(self):  # sparsematrix.rs:263-271
        out = C.c_int(0)
        check(lib().smh_crs_is_sorted(self._h, C.byref(out)))
        return bool(out.value)

    def sort_rows(self):
        """Sortable::sort_row (sparsemat_crs.rs:163-172) on every row: ascending columns, stable."""
        check(lib().smh_crs_sort_rows(self._h))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().smh_crs_destroy(h)
            except Exception:
                pass

    # ---- SparseMatrix accessors (sparsemat_crs.rs:124-134) ------------------------------------
    @property
    def dtype(self):
        return self._dtype

    def n_rows(self):
        return lib().smh_crs_n_rows(self._h)

    def n_cols(self):
        return lib().smh_crs_n_cols(self._h)

    def n_non_zero_entries(self):
        """Entries the handle's arrays hold.  The reference's ``n_non_zero_entries()`` (``columns.len()``) additionally counts
        an entry orphaned by the first-push quirk of a replay / transpose / prod: add ``orphans()``."""
        return lib().smh_crs_nnz(self._h)

    def orphans(self):
        """0 or 1: the entry the reference's container would still hold although no row reaches it (``smh_crs_orphans``)."""
        return lib().smh_crs_orphans(self._h)

    def empty(self):  # sparsematrix.rs:119-121
        return self.n_rows() == 0

    def density(self):  # sparsematrix.rs:237-241
        return self.n_non_zero_entries() / (self.n_rows() * self.n_cols())

    def sparsity(self):  # sparsematrix.rs:243-246
        return 1.0 - self.density()

    def raw_parts(self):
        off = np.empty(self.n_rows() + 1, dtype=np.uint32)
        col = np.empty(self.n_non_zero_entries(), dtype=np.uint32)
        val = np.empty(self.n_non_zero_entries(), dtype=self._dtype)
        check(lib().smh_crs_download(self._h, off.ctypes.data, col.ctypes.data, val.ctypes.data))
        return off, col, val

    def iter_row(self, row):  # sparsemat_crs.rs:102-110 (row >= n_rows -> empty)
        if row >= self.n_rows():
            return []
        off, col, val = self.raw_parts()
        return list(zip(col[off[row]:off[row + 1]], val[off[row]:off[row + 1]]))

    def scale(self, a):  # sparsemat_crs.rs:153-157
        check(lib().smh_crs_scale(self._h, float(a)))

    def update_values(self, values):
        values = np.ascontiguousarray(values, dtype=self._dtype)
        assert len(values) == self.n_non_zero_entries()
        check(lib().smh_crs_update_values(self._h, values.ctypes.data))

    # ---- kernel selection ----------------------------------------------------------------------
    def resolved_variant(self):
        v, lanes = C.c_int(), C.c_int()
        check(lib().smh_crs_resolved_variant(self._h, C.byref(v), C.byref(lanes)))
        return {1: "vector", 2: "merge", 3: "seq", 4: "stream", 5: "colblock", 6: "colfused", 7: "colsplit", 8: "tiled"}[v.value], lanes.value

    def set_colblock_shift(self, shift):
        """K2c: column blocks of 2**shift columns (0: automatic, 2 MiB of x)."""
        check(lib().smh_crs_set_colblock_shift(self._h, shift))

    def tiled_layout(self, arrays=False):
        """K2t (``smh_crs_tiled_layout``; builds the 2-D tiled copy on first use): dict with n_slices, slice_columns,
        rows_per_block, n_row_blocks, copy_entries, n_products; with ``arrays`` also the plan's arrays
        (``smh_crs_tiled_array``): slice_chunks, chunks (n x 2: first product slot, entries), codes, values, product_rows,
        row_block_start, tile_start ((n_row_blocks + 1) x n_slices), products (of the last launch)."""
        a, b, c, d, e, f = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t(), C.c_size_t()
        check(lib().smh_crs_tiled_layout(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)))
        check(lib().smh_crs_tiled_products(self._h, C.byref(f)))
        out = {"n_slices": a.value, "slice_columns": b.value, "rows_per_block": c.value, "n_row_blocks": d.value, "copy_entries": e.value,
               "n_products": f.value}
        if arrays:
            kinds = (("slice_chunks", np.uint32), ("chunks", np.uint32), ("codes", np.uint16), ("values", self.dtype), ("product_rows", np.uint16),
                     ("row_block_start", np.uint32), ("tile_start", np.uint32), ("products", self.dtype))
            for which, (name, dt) in enumerate(kinds):
                n = C.c_size_t()
                check(lib().smh_crs_tiled_array(self._h, which, None, 0, C.byref(n)))
                buf = np.empty(n.value // np.dtype(dt).itemsize, dtype=dt)
                check(lib().smh_crs_tiled_array(self._h, which, buf.ctypes.data, buf.nbytes, None))
                out[name] = buf
            out["chunks"] = out["chunks"].reshape(-1, 2)
            out["tile_start"] = out["tile_start"].reshape(d.value + 1, a.value)
        return out

    def colsplit_flag(self):
        """True when the handle keeps a row-length split (builds it on first use)."""
        flag = C.c_int()
        check(lib().smh_crs_colsplit(self._h, C.byref(flag), None, None, None, None, None))
        return bool(flag.value)

    def colsplit(self):
        """The row-length split (``smh_crs_colsplit``): dict with split (bool), min_long, n_long, long_rows and the two
        sub-matrices' raw parts ``long`` / ``short`` = (n_rows, offsets, columns, values)."""
        flag, ml, nl = C.c_int(), C.c_uint32(), C.c_size_t()
        check(lib().smh_crs_colsplit(self._h, C.byref(flag), C.byref(ml), C.byref(nl), None, None, None))
        out = {"split": bool(flag.value), "min_long": ml.value, "n_long": nl.value}
        if out["split"]:
            rows = np.zeros(nl.value, np.uint32)
            hl, hs = C.c_void_p(), C.c_void_p()
            check(lib().smh_crs_colsplit(self._h, None, None, None, rows.ctypes.data, C.byref(hl), C.byref(hs)))
            out["long_rows"] = rows
            for name, h in (("long", hl), ("short", hs)):
                nr, nnz = lib().smh_crs_n_rows(h), lib().smh_crs_nnz(h)
                off, col, val = np.zeros(nr + 1, np.uint32), np.zeros(nnz, np.uint32), np.zeros(nnz, self._dtype)
                check(lib().smh_crs_download(h, off.ctypes.data, col.ctypes.data if nnz else None, val.ctypes.data if nnz else None))
                var, lanes = C.c_int(), C.c_int()
                check(lib().smh_crs_resolved_variant(h, C.byref(var), C.byref(lanes)))
                out[name] = (nr, off, col, val)
                out[name + "_variant"] = {1: "vector", 2: "merge", 3: "seq", 4: "stream", 5: "colblock", 6: "colfused", 7: "colsplit", 8: "tiled"}[var.value]
        return out

    def colfused(self, arrays=True):
        """The K2f copy (``smh_crs_colfused``): dict with fits, shift, n_blocks, rows_per_lane, n_tiles and -- with
        ``arrays`` -- tile_rows, segments, counts, columns, values (entries sorted by (tile, block, row, storage order))."""
        fits, sh, nb, rt, nt = C.c_int(), C.c_uint32(), C.c_size_t(), C.c_uint32(), C.c_size_t()
        check(lib().smh_crs_colfused(self._h, C.byref(fits), C.byref(sh), C.byref(nb), C.byref(rt), C.byref(nt), None, None, None, None, None))
        out = {"fits": bool(fits.value), "shift": sh.value, "n_blocks": nb.value, "rows_per_lane": rt.value, "n_tiles": nt.value}
        if arrays and out["fits"]:
            nnz = self.n_non_zero_entries()
            tiles = np.zeros(nt.value + 1, np.uint32)
            seg = np.zeros(nt.value * nb.value + 1, np.uint32)
            cnt = np.zeros(nt.value * nb.value * 64 * rt.value, np.uint8)
            col = np.zeros(nnz, np.uint32)
            val = np.zeros(nnz, self._dtype)
            check(lib().smh_crs_colfused(self._h, None, None, None, None, None, tiles.ctypes.data, seg.ctypes.data,
                                         cnt.ctypes.data if len(cnt) else None, col.ctypes.data if nnz else None,
                                         val.ctypes.data if nnz else None))
            out.update(tile_rows=tiles, segments=seg, counts=cnt, columns=col, values=val)
        return out

    def colblock(self, arrays=True):
        """K2c column-blocked copy: dict(shift, n_blocks, rows_per_thread, span_fraction[, offsets[B, n_rows+1],
        columns, values])."""
        sh, nb, rpt, span = C.c_uint32(), C.c_size_t(), C.c_int(), C.c_double()
        check(lib().smh_crs_colblock(self._h, C.byref(sh), C.byref(nb), C.byref(rpt), C.byref(span), None, None, None))
        out = dict(shift=sh.value, n_blocks=nb.value, rows_per_thread=rpt.value, span_fraction=span.value)
        if arrays:
            nnz = self.n_non_zero_entries()
            off = np.zeros((nb.value, self.n_rows() + 1), dtype=np.uint32)
            col = np.zeros(nnz, dtype=np.uint32)
            val = np.zeros(nnz, dtype=self._dtype)
            check(lib().smh_crs_colblock(self._h, None, None, None, None, off.ctypes.data,
                                         col.ctypes.data if nnz else None, val.ctypes.data if nnz else None))
            out.update(offsets=off, columns=col, values=val)
        return out

    def set_vector_lanes(self, lanes):
        check(lib().smh_crs_set_vector_lanes(self._h, lanes))

    def set_stream_xs(self, mode):
        """K1s XS (the tile's column intervals of x staged in LDS): -1 automatic, 0 never, 1 whenever the tiles allow."""
        check(lib().smh_crs_set_stream_xs(self._h, mode))

    def set_stream_direct(self, mode):
        """K1s XD (stage offsets instead of column codes, unskewed product stage): -1 automatic, 0 never, 1 whenever x is staged."""
        check(lib().smh_crs_set_stream_direct(self._h, mode))

    def stream_direct(self):
        """Does a STREAM launch of this matrix run as K1s XD?"""
        a = C.c_int()
        check(lib().smh_crs_stream_direct(self._h, C.byref(a)))
        return bool(a.value)

    def stream_value_dict(self):
        """K1s XD-V (``smh_crs_stream_value_dict``): the dictionary of the matrix's distinct values the CSR-stream kernel multiplies
        with instead of reading the value array -- a numpy array of its entries, empty when the form is not active (more than 32 / 16
        distinct values, or no stage-offset codes)."""
        n = C.c_int()
        buf = np.zeros(32, dtype=self.dtype)
        check(lib().smh_crs_stream_value_dict(self._h, C.byref(n), buf.ctypes.data))
        return buf[:n.value].copy()

    def set_stream_value_dict(self, mode):
        """-1 automatic (whenever the values allow), 0 never (``smh_crs_set_stream_value_dict``)."""
        check(lib().smh_crs_set_stream_value_dict(self._h, int(mode)))

    def stream_layout(self):
        """What a STREAM launch of this matrix uses: dict(coded, byte_lengths, small_tiles, xs_chunks)."""
        a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(lib().smh_crs_stream_layout(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"coded": bool(a.value), "byte_lengths": bool(b.value), "small_tiles": bool(c.value), "xs_chunks": d.value}

    def set_vector_chunks(self, chunks):
        check(lib().smh_crs_set_vector_chunks(self._h, chunks))

    def set_ring(self, mode):
        """K1r (LDS x-ring) for the vector family: -1 automatic, 0 off, 1 on."""
        check(lib().smh_crs_set_ring(self._h, mode))

    def ring_entries(self):
        """Columns the LDS ring of this matrix's K1r plan holds (16384, or 32768 for f32 matrices that need it)."""
        out = C.c_uint32()
        check(lib().smh_crs_ring_entries(self._h, C.byref(out)))
        return out.value

    def ring_column_form(self):
        """What K1r's ring phases stream for their columns under the current settings: "u32", "col16" or "col12" (the compact
        12-bit form: f32 on the single-window 16384-column ring).  "u32" also when the ring kernel is not in use."""
        out = C.c_int()
        check(lib().smh_crs_ring_column_form(self._h, C.byref(out)))
        return ("u32", "col16", "col12")[out.value]

    def ring_value_form(self):
        """What K1r's ring phases stream for their values under the current settings: ("val24", E) -- 24-bit fixed-point values
        k * 2^E in 16-byte chunk records, taken with the compact column form when every value fits --, ("plain", None) -- the value
        array --, or ("refused", None): the value array, the matrix was tested and some value does not fit."""
        form, exp = C.c_int(), C.c_int()
        check(lib().smh_crs_ring_values(self._h, C.byref(form), C.byref(exp)))
        return ("val24", exp.value) if form.value == 1 else ("refused" if form.value < 0 else "plain", None)

    def ring_bands(self, intervals=False):
        """1 (one sliding window) or 4 (banded ring); with ``intervals`` also the per-tile column intervals
        [n_tiles64, 4, 2] of a banded plan (None otherwise)."""
        bands = C.c_uint32()
        check(lib().smh_crs_ring_bands(self._h, C.byref(bands), None))
        if not intervals:
            return bands.value
        if bands.value != 4:
            return bands.value, None
        table = np.zeros(((self.n_rows() + 63) // 64, 4, 2), dtype=np.uint32)
        check(lib().smh_crs_ring_bands(self._h, C.byref(bands), table.ctypes.data))
        return bands.value, table

    def ring_plan(self):
        """(n_blocks, ring_fraction, active, phase_ptr, phases[n,11]) of the K1r plan; a phase row is
        (row_begin, row_end, load_lo, load_hi, use_ring, lo1, lo2, lo3, hi1, hi2, hi3)."""
        nb, nph, frac, act = C.c_uint32(), C.c_size_t(), C.c_double(), C.c_int()
        check(lib().smh_crs_ring_plan(self._h, C.byref(nb), C.byref(nph), C.byref(frac), C.byref(act), None, None))
        ptr = np.zeros(nb.value + 1, dtype=np.uint32)
        ph = np.zeros((nph.value, 11), dtype=np.uint32)
        check(lib().smh_crs_ring_plan(self._h, None, None, None, None, ptr.ctypes.data,
                                      ph.ctypes.data if nph.value else None))
        return nb.value, frac.value, bool(act.value), ptr, ph

    def ring_regular(self):
        """One u32 per phase of ``ring_plan()``: the row length L of a ring phase (use_ring == 1) whose rows are all L > 0 entries
        long, else 0.  Where every phase gathers from the ring and the ring phases stream 16-bit or 12-bit columns, the ring
        kernel computes such a phase's row offsets instead of loading them (SMH_RING_REGULAR=0: never); results do not change."""
        nph = C.c_size_t()
        check(lib().smh_crs_ring_plan(self._h, None, C.byref(nph), None, None, None, None))
        out = np.zeros(nph.value, dtype=np.uint32)
        if nph.value:
            check(lib().smh_crs_ring_regular(self._h, out.ctypes.data))
        return out

    def ring_launch_form(self):
        """(form, threads, resident_per_cu) of the ring kernel a plain product would launch now, under the current settings and
        knobs: form 0 = the three bodies, 1 = the regular and the loading ring body, 2 = the all-regular form (f32, every phase
        regular: 768-thread workgroups; SMH_RING_ALLREG=0: form 1 instead), -1 = the ring kernel is not in use; the workgroup size;
        and how many such workgroups a compute unit holds at once (the runtime's occupancy answer).  Results do not depend on it."""
        form, threads, resident = C.c_int(), C.c_int(), C.c_int()
        check(lib().smh_crs_ring_launch_form(self._h, C.byref(form), C.byref(threads), C.byref(resident)))
        return form.value, threads.value, resident.value

    def max_row_len(self):
        out = C.c_uint32()
        check(lib().smh_crs_max_row_len(self._h, C.byref(out)))
        return out.value

    def col_range(self):
        """(smallest, largest) stored column index."""
        lo, hi = C.c_uint32(), C.c_uint32()
        check(lib().smh_crs_col_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def merge_table(self):
        n = lib().smh_crs_merge_tiles(self._h)
        rows = np.zeros(n + 1, dtype=np.uint32)
        nz = np.zeros(n + 1, dtype=np.uint32)
        check(lib().smh_crs_merge_table(self._h, rows.ctypes.data, nz.ctypes.data))
        return rows, nz, lib().smh_crs_merge_tile_items(self._h)

    # ---- SparseMatrix::mvp (sparsematrix.rs:146-158) and `A * v` (:435-443) --------------------
    def mvp(self, rhs, variant="auto"):
        """y = A.rhs; returns a NEW vector with dim == n_rows.  ``rhs`` is a DenseVec (device
        resident) or anything array-like (host: uploaded, result returned as numpy)."""
        var = _lib.VARIANTS[variant]
        if isinstance(rhs, DenseVec):
            ret = DenseVec.zeros(self.n_rows(), self._dtype)
            check(lib().smh_crs_spmv_vec(self._h, rhs._h, ret._h, var))
            return ret
        x = np.ascontiguousarray(rhs, dtype=self._dtype)
        y = np.zeros(self.n_rows(), dtype=self._dtype)
        check(lib().smh_crs_spmv(self._h, x.ctypes.data if x.size else None, x.size,
                                 y.ctypes.data if y.size else None, var))
        return y

    def mvp_many(self, rhs):
        """Y = A.X for k right-hand sides in one sweep over the matrix (``smh_crs_spmv_many``): column c of the result is bit for bit
        ``mvp(x_c, variant="seq")``.  A MultiVec (device resident) gives a NEW MultiVec; a 2-D array-like of shape (k, x_len) gives a
        numpy array of shape (k, n_rows)."""
        if isinstance(rhs, MultiVec):
            ret = MultiVec.zeros(self.n_rows(), rhs.count(), self._dtype)
            check(lib().smh_crs_spmv_many(self._h, rhs._h, ret._h))
            return ret
        x = pack_host(rhs, self._dtype)
        y = np.zeros((x.shape[0], self.n_rows()), dtype=self._dtype)
        check(lib().smh_crs_spmv_many_host(self._h, x.ctypes.data if x.size else None, x.shape[1], x.shape[0],
                                           y.ctypes.data if y.size else None))
        return y

    def mvp_many_dev(self, x_ptr, x_len, y_ptr, k, ld, stream=None):
        """Asynchronous Y = A.X on raw interleaved device pointers (16-byte aligned; ``ld`` a multiple of 4, at least ``k``)."""
        check(lib().smh_crs_spmv_many_dev(self._h, C.c_void_p(x_ptr), x_len, C.c_void_p(y_ptr), k, ld, C.c_void_p(stream or 0)))

    def __mul__(self, rhs):
        """``A * v`` (sparsematrix.rs:435-443): mvp; ``A * s`` for a scalar s (Mul<T>, :422-432): a scaled clone."""
        if isinstance(rhs, numbers.Real):
            ret = self.clone()
            ret.scale(rhs)
            return ret
        return self.mvp(rhs)

    def __imul__(self, rhs):  # MulAssign<T> (:389-395): scale in place
        if isinstance(rhs, numbers.Real):
            self.scale(rhs)
            return self
        return NotImplemented

    def inner_prod(self, lhs, rhs, variant="auto"):
        """SparseMatrix::inner_prod (sparsematrix.rs:161-171): lhs^T A rhs as a Python float."""
        out = C.c_double()
        var = _lib.VARIANTS[variant]
        if isinstance(lhs, DenseVec) and isinstance(rhs, DenseVec):
            check(lib().smh_crs_inner_prod_vec(self._h, lhs._h, rhs._h, var, C.byref(out)))
            return out.value
        a = np.ascontiguousarray(lhs, dtype=self._dtype)
        b = np.ascontiguousarray(rhs, dtype=self._dtype)
        check(lib().smh_crs_inner_prod(self._h, a.ctypes.data if a.size else None, a.size,
                                       b.ctypes.data if b.size else None, b.size, var, C.byref(out)))
        return out.value

    def eigsh(self, k=6, which="LA", ncv=None, tol=0.0, maxiter=None, v0=None, return_eigenvectors=True, variant="auto"):
        """The k algebraically largest (``which="LA"``) or smallest ("SA") eigenpairs of a SYMMETRIC matrix by thick-restart Lanczos
        with full reorthogonalisation -- an EXTENSION (``smh_eigsh_vec``; the reference has no eigensolver).  Symmetry is the
        caller's promise, as it is for ``ConjugateGradient``: nothing checks it.  A multiple eigenvalue is found once.
        ``ncv``: the columns of the basis, k + 2 .. 128 after clipping to the dimension (None: min(n, max(2 k + 1, 20)));
        ``tol``: pair i is converged when its estimate is at most tol * max|theta| (0 stands for 2^10 eps of the matrix dtype);
        ``maxiter``: the restarts allowed (None: 1000); ``v0``: the start, a DenseVec or array-like (None:
        ``numpy.random.default_rng(0).standard_normal(n)`` -- the library itself draws no random numbers).
        Returns an ``EigshResult``: ``values`` (f64, wanted-first), ``vectors`` (a MultiVec of k columns, not renormalised; None
        without ``return_eigenvectors``), ``estimates``, ``n_conv`` (the converged prefix; < k when ``maxiter`` ran out: the k
        best pairs are returned all the same), ``restarts``, ``products`` and ``breakdown`` (0; 1: the Krylov space is exhausted,
        the pairs that exist are exact; 2: a zero or non-finite start; 3: non-finite data -- 2 and 3 return no pairs: ``values``,
        ``vectors`` and ``estimates`` are None)."""
        n, k = self.n_rows(), int(k)
        if which not in _lib.EIGSH_WHICH:
            raise ValueError('which must be "LA" or "SA"')
        if v0 is None:
            v0 = np.random.default_rng(0).standard_normal(n)
        start = v0 if isinstance(v0, DenseVec) else DenseVec.from_vec(np.ascontiguousarray(v0, dtype=self._dtype))
        if tol == 0.0:
            tol = 1024.0 * float(np.finfo(self._dtype).eps)
        vectors = MultiVec.zeros(n, k, self._dtype) if return_eigenvectors and 0 < k <= n else None
        values, estimates = np.zeros(max(k, 1), np.float64), np.zeros(max(k, 1), np.float64)
        n_conv, restarts, products, brk = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int()
        dp = C.POINTER(C.c_double)
        check(lib().smh_eigsh_vec(self._h, start._h, vectors._h if vectors is not None else None, k, int(ncv or 0), _lib.EIGSH_WHICH[which],
                                  float(tol), 1000 if maxiter is None else int(maxiter), _lib.VARIANTS[variant], values.ctypes.data_as(dp),
                                  estimates.ctypes.data_as(dp), C.byref(n_conv), C.byref(restarts), C.byref(products), C.byref(brk)))
        nothing = brk.value in (2, 3)
        return EigshResult(None if nothing else values[:k], None if nothing else vectors, None if nothing else estimates[:k], n_conv.value,
                           restarts.value, products.value, brk.value)

    def prepare(self, variant="auto"):
        """Build the lazily created workspaces of ``variant`` now (before capturing mvp_dev into a hipGraph)."""
        check(lib().smh_crs_prepare(self._h, _lib.VARIANTS[variant]))

    def prepare_stats(self, variant="auto"):
        """``smh_crs_prepare_stats``: (prepare_ms, derived_bytes) -- what the inspectors of ``variant`` cost: host wall time of
        the create-time inspection plus the plan's build, and the device memory they hold beside the CRS arrays.  The reference
        has no set-up step (sparsemat_crs.rs:102-110)."""
        ms, nb = C.c_double(), C.c_size_t()
        check(lib().smh_crs_prepare_stats(self._h, _lib.VARIANTS[variant], C.byref(ms), C.byref(nb)))
        return ms.value, nb.value

    def mvp_dev(self, x_ptr, x_len, y_ptr, variant="auto", stream=None):
        """Asynchronous y = A.x on raw device pointers (stream: a hipStream_t value or None)."""
        check(lib().smh_crs_spmv_dev(self._h, C.c_void_p(x_ptr), x_len, C.c_void_p(y_ptr),
                                     _lib.VARIANTS[variant], C.c_void_p(stream or 0)))


class UpdatePlan:
    """The targets and the sorted order of one (rows, cols, ops) stream on one SparseMatCRS (``smh_update_plan``):
    ``execute(values)`` is what ``apply(rows, cols, values, ops)`` leaves, bit for bit, in one gather-and-fold pass.  Holds its
    matrix, so the matrix cannot be collected first."""

    def __init__(self, handle, matrix, n_ops):
        self._h = handle
        self._m = matrix
        self._n = n_ops

    def execute(self, values, from_zero=False):
        """Folds ``values`` (one per operation, stream order) into the matrix.  ``from_zero``: every targeted entry starts
        from +0 instead of its stored value ("zero, then assemble" in one pass); untargeted entries are not touched."""
        values = np.asarray(values)
        dtype = self._m._dtype
        if values.dtype.kind == "f" and values.dtype != dtype:
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "values are %s, the matrix holds %s" % (values.dtype, dtype))
        values = np.ascontiguousarray(values, dtype=dtype)
        if len(values) != self._n:
            raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "the plan holds %d operations, values has %d" % (self._n, len(values)))
        check(lib().smh_update_plan_execute(self._h, self._m._h, values.ctypes.data if self._n else None, 1 if from_zero else 0))

    def execute_dev(self, vals_ptr, from_zero=False):
        """``execute`` over a value array that already lives in HBM (raw device pointer)."""
        check(lib().smh_update_plan_execute_dev(self._h, self._m._h, C.c_void_p(vals_ptr or 0), 1 if from_zero else 0))

    def stats(self):
        """``smh_update_plan_stats`` as a dict: n_ops, n_targets, n_live_ops, longest_run, long_run_threshold, device_bytes."""
        names = ("n_ops", "n_targets", "n_live_ops", "longest_run", "long_run_threshold", "device_bytes")
        out = [C.c_size_t(0) for _ in names]
        check(lib().smh_update_plan_stats(self._h, *[C.byref(o) for o in out]))
        return {k: int(o.value) for k, o in zip(names, out)}

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().smh_update_plan_destroy(h)
            except Exception:
                pass
