"""MultiVec: k ``DenseVec``s of one dimension held against one matrix (load cases, block Krylov methods, subspace
iteration), backed by a device-resident ``smh_mvec``.

The reference has no such type -- its ``SparseMatrix::mvp`` (sparsematrix.rs:146-158) is generic over the vector and is
called once per right-hand side; ``SparseMatCRS.mvp_many`` gives the same k results, bit for bit, from one sweep over the
matrix.  On the device the vectors are interleaved (element i of vector c at ``[i * ld + c]``, ``ld = leading_dim(k)``); on
the host a MultiVec is a ``(k, n)`` array: row c is vector c.  Both transpositions run in the HIP library.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .densevec import DenseVec


def leading_dim(k):
    """Columns of the interleaved storage of k vectors: k rounded up to a multiple of 4 (the padding columns stay zero)."""
    return (int(k) + 3) // 4 * 4


def pack_host(vecs, dtype=None):
    """The host format of the C ABI -- k vectors of n entries, one after the other -- as one contiguous ``(k, n)`` array,
    from a 2-D array-like or a list of equally long 1-D array-likes."""
    rows = [np.asarray(v) for v in vecs] if isinstance(vecs, (list, tuple)) else None
    if rows is not None and len({r.shape for r in rows}) > 1:
        raise _lib.SparseMatPanic(_lib.SMH_ERR_DIM_MISMATCH, "Dimension mismatch")
    a = np.asarray(rows if rows is not None else vecs)
    if dtype is None:
        dtype = a.dtype if a.dtype in (np.float32, np.float64) else np.float64
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.ndim != 2:
        raise _lib.SparseMatPanic(_lib.SMH_ERR_INVALID, "a multi-vector is a (k, n) array (got %d dimensions)" % a.ndim)
    return a


def unpack_host(flat, k, n):
    """The ``(k, n)`` view of a buffer in the host format."""
    return np.asarray(flat).reshape(k, n)


class MultiVec:
    __slots__ = ("_h", "_dtype")

    def __init__(self, handle, dtype):
        self._h = handle
        self._dtype = np.dtype(dtype)

    @classmethod
    def from_vecs(cls, vecs, dtype=None):
        """From a 2-D array-like of shape (k, n), or a list of 1-D array-likes or DenseVecs (device to device)."""
        if isinstance(vecs, (list, tuple)) and len(vecs) and all(isinstance(v, DenseVec) for v in vecs):
            ret = cls.zeros(vecs[0].dim(), len(vecs), vecs[0].dtype if dtype is None else dtype)
            for c, v in enumerate(vecs):
                ret.set_column(c, v)
            return ret
        a = pack_host(vecs, dtype)
        h = C.c_void_p()
        check(lib().smh_mvec_from_host(_lib.dtype_code(a.dtype), a.shape[1], a.shape[0], a.ctypes.data if a.size else None, C.byref(h)))
        return cls(h, a.dtype)

    @classmethod
    def zeros(cls, n, k, dtype=np.float32):
        h = C.c_void_p()
        check(lib().smh_mvec_create(_lib.dtype_code(dtype), n, k, C.byref(h)))
        return cls(h, dtype)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().smh_mvec_destroy(h)
            except Exception:
                pass

    @property
    def dtype(self):
        return self._dtype

    def dim(self):
        return lib().smh_mvec_dim(self._h)

    def count(self):
        return lib().smh_mvec_count(self._h)

    def ld(self):
        return lib().smh_mvec_ld(self._h)

    def data_ptr(self):
        """The interleaved device storage: dim() * ld() elements."""
        return lib().smh_mvec_data(self._h)

    def to_numpy(self):
        out = np.empty(self.count() * self.dim(), dtype=self._dtype)
        check(lib().smh_mvec_download(self._h, out.ctypes.data if out.size else None))
        return unpack_host(out, self.count(), self.dim())

    def column(self, c):
        """Vector c as a new DenseVec."""
        ret = DenseVec.zeros(self.dim(), self._dtype)
        check(lib().smh_mvec_get_column(self._h, c, ret._h))
        return ret

    def set_column(self, c, v):
        if not isinstance(v, DenseVec):
            v = DenseVec.from_vec(v, self._dtype)
        check(lib().smh_mvec_set_column(self._h, c, v._h))

    # ---- the per-column BLAS-1 (densevec.rs:51-73, vector.rs:50-58, k times): in place, one rounding per operation ----
    def copy(self):
        """A new MultiVec with the same vectors (clone(), densevec.rs:9 derive)."""
        ret = MultiVec.zeros(self.dim(), self.count(), self._dtype)
        check(lib().smh_mvec_copy(ret._h, self._h))
        return ret

    def add(self, other):
        check(lib().smh_mvec_add(self._h, other._h))
        return self

    def sub(self, other):
        check(lib().smh_mvec_sub(self._h, other._h))
        return self

    def scale(self, factors):
        """Column c times ``factors[c]`` (k factors; a scalar scales every column)."""
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(factors, np.float64), (self.count(),)))
        check(lib().smh_mvec_scale(self._h, a.ctypes.data_as(C.POINTER(C.c_double))))
        return self

    def dot(self, other):
        """The k dot products of the columns, as a numpy f64 array (each summed in a fixed order that depends on dim() alone)."""
        out = np.zeros(self.count(), np.float64)
        check(lib().smh_mvec_dot(self._h, other._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def norm_squared(self):
        out = np.zeros(self.count(), np.float64)
        check(lib().smh_mvec_norm_squared(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out
