"""CPU: the multi-vector additions to the C ABI are declared, bound and exported; without a device they fail loudly (no CPU
fallback) and report argument errors first; the Python side's (k, n) host format round-trips; ld = 4 * ceil(k / 4)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sparsemat_amd as sm
from sparsemat_amd import _lib, multivec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sparsemat_hip.h")
NEW_SYMBOLS = ["smh_mvec_create", "smh_mvec_from_host", "smh_mvec_upload", "smh_mvec_download", "smh_mvec_destroy", "smh_mvec_dim",
               "smh_mvec_count", "smh_mvec_ld", "smh_mvec_dtype", "smh_mvec_data", "smh_mvec_set_column", "smh_mvec_get_column",
               "smh_crs_spmv_many", "smh_crs_spmv_many_dev", "smh_crs_spmv_many_host"]


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(smh_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", sm.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (smh_[a-z0-9_]+)", out))
    L = sm.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
        assert name in exported, name
    assert L.smh_abi_version() == 3  # additions only
    assert sm.MultiVec is multivec.MultiVec and "MultiVec" in sm.__all__ and hasattr(sm.SparseMatCRS, "mvp_many")


def test_k_zero_is_refused_before_the_device_is_asked_for():
    h = C.c_void_p()
    for dtype in (_lib.SMH_F32, _lib.SMH_F64):
        assert sm.lib().smh_mvec_create(dtype, 5, 0, C.byref(h)) == _lib.SMH_ERR_INVALID
        assert b"k == 0" in sm.lib().smh_last_error() and not h.value
    assert sm.lib().smh_mvec_create(7, 5, 1, C.byref(h)) == _lib.SMH_ERR_INVALID            # a dtype that is none
    assert sm.lib().smh_mvec_create(_lib.SMH_F64, 1 << 62, 4, C.byref(h)) == _lib.SMH_ERR_INVALID  # n * ld * 8 overflows
    assert b"address space" in sm.lib().smh_last_error()
    x = np.zeros(4, np.float32)
    assert sm.lib().smh_crs_spmv_many_host(None, x.ctypes.data, 4, 0, x.ctypes.data) == _lib.SMH_ERR_INVALID
    assert sm.lib().smh_crs_spmv_many_dev(None, None, 4, None, 0, 0, None) == _lib.SMH_ERR_INVALID


def _no_gpu():
    n = C.c_int(0)
    sm.lib().smh_device_count(C.byref(n))
    return n.value == 0


@pytest.mark.skipif(not _no_gpu(), reason="only meaningful on a box without a GPU")
def test_multivec_and_mvp_many_fail_loudly_without_a_device():
    with pytest.raises(sm.SparseMatPanic) as e:
        sm.MultiVec.zeros(5, 3, np.float32)
    assert e.value.status == _lib.SMH_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(sm.SparseMatPanic) as e:
        sm.MultiVec.from_vecs(np.ones((2, 3), np.float64))
    assert e.value.status == _lib.SMH_ERR_NO_DEVICE
    # no matrix can exist on this box: the host-pointer entry is reached through a shell without a handle
    with pytest.raises(sm.SparseMatPanic) as e:
        sm.SparseMatCRS(None, np.float32).mvp_many(np.ones((2, 3), np.float32))
    assert e.value.status == _lib.SMH_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


def test_host_format_round_trips():
    rng = np.random.default_rng(5)
    for dtype in (np.float32, np.float64):
        for k, n in [(1, 7), (3, 5), (4, 1), (9, 0), (5, 130)]:
            a = rng.uniform(-1, 1, (k, n)).astype(dtype)
            for form in (a, [row for row in a], [list(row) for row in a], np.asfortranarray(a)):
                p = multivec.pack_host(form, dtype)
                assert p.shape == (k, n) and p.dtype == dtype and p.flags.c_contiguous
                # the C ABI's host format: vector c occupies [c * n, (c + 1) * n)
                flat = p.reshape(-1)
                for c in range(k):
                    assert np.array_equal(flat[c * n:(c + 1) * n], a[c])
                assert np.array_equal(multivec.unpack_host(flat.copy(), k, n), a)
    assert multivec.pack_host([[1, 2], [3, 4]]).dtype == np.float64  # integers: the wider type, like DenseVec.from_vec
    with pytest.raises(sm.SparseMatPanic) as e:
        multivec.pack_host(np.ones(4, np.float32))
    assert e.value.status == _lib.SMH_ERR_INVALID
    with pytest.raises(sm.SparseMatPanic) as e:
        multivec.pack_host([np.ones(4), np.ones(5)])
    assert e.value.status == _lib.SMH_ERR_DIM_MISMATCH


def test_leading_dimension():
    ks = np.arange(1, 10)
    want = 4 * np.ceil(ks / 4).astype(np.int64)   # k rounded up to a multiple of 4
    assert list(want) == [4, 4, 4, 4, 8, 8, 8, 8, 12]
    assert [multivec.leading_dim(int(k)) for k in ks] == list(want)
