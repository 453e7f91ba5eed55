#!/usr/bin/env python3
"""Times SparseMatrix::add / sub of SparseMatCRS on one GPU (development aid, not the contract bench): every route of
csrc/matadd.hip on the shapes DESIGN.md §4 names, with smh_crs_transpose of the same matrix as the yardstick.

  (a) 512^3 7-point Laplacian f32: A + A and A -= A (same pattern);
  (b) the same A plus a diagonal-only matrix that shifts the diagonal (structure unchanged);
  (c) the C3 shape -- f64 power law 1-2048 (alpha 1.52), 10 M rows -- plus its transpose (general route, long rows).

Each call is synchronous; HIP events on the null stream bracket it, so a figure is the whole call: count pass, scan, emit
and the create-time inspection of the result handle.  Algorithmic bytes = the CRS arrays of a and b read once plus the
result's arrays written once (in place and structure unchanged: the values alone written).

    python tools/add_bench.py [--grid 512] [--c3-rows 10000000] [--reps 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import synth  # noqa: E402
from sparsemat_amd._lib import check, lib  # noqa: E402

PEAK_GB_S = 8000.0


def crs_bytes(m):
    return 4 * (m.n_rows() + 1) + (4 + m.dtype.itemsize) * m.n_non_zero_entries()


def timed(fn, reps):
    """median and best ms of `fn` (which returns whatever must stay alive until after the stop event)"""
    e0, e1 = C.c_void_p(), C.c_void_p()
    check(lib().smh_event_create(C.byref(e0)))
    check(lib().smh_event_create(C.byref(e1)))
    ts, keep = [], None
    try:
        for _ in range(reps):
            keep = None
            check(lib().smh_event_record(e0, None))
            keep = fn()
            check(lib().smh_event_record(e1, None))
            ms = C.c_float()
            check(lib().smh_event_elapsed_ms(e0, e1, C.byref(ms)))
            ts.append(ms.value)
    finally:
        lib().smh_event_destroy(e0)
        lib().smh_event_destroy(e1)
    ts.sort()
    return ts[len(ts) // 2], ts[0], keep


def report(name, ms, best, nbytes, route, extra=None):
    line = {"case": name, "route": route, "ms": round(ms, 3), "best_ms": round(best, 3), "algorithmic_GB": round(nbytes / 1e9, 3),
            "GB_per_s": round(nbytes / 1e6 / ms, 1), "fraction_of_8TB_s": round(nbytes / 1e6 / ms / PEAK_GB_S, 3)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--c3-rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    n_dev = C.c_int()
    check(lib().smh_device_count(C.byref(n_dev)))
    assert n_dev.value > 0, "needs a HIP device"
    route = sm.SparseMatCRS.last_add_route

    # (a) / (b): the 7-point Laplacian
    g = args.grid
    a = synth.crs_laplace3d(g, g, g, np.float32)
    n = a.n_rows()
    ab = crs_bytes(a)
    ms, best, _ = timed(lambda: a.transpose(), args.reps)
    report("(a) transpose(A) yardstick, %d^3 f32" % g, ms, best, 2 * ab, sm.SparseMatCRS.last_transpose_route())
    ms, best, _ = timed(lambda: a + a, args.reps)
    report("(a) A + A, %d^3 f32" % g, ms, best, 3 * ab, route())
    c = a.clone()
    ms, best, _ = timed(lambda: c.sub(c), args.reps)
    report("(a) A -= A in place, %d^3 f32" % g, ms, best, 2 * ab + 4 * a.n_non_zero_entries(), route())
    del c
    d_off = synth.DeviceBuffer((n + 1) * 4)
    d_off.upload(np.arange(n + 1, dtype=np.uint32))
    d_col = synth.DeviceBuffer((n + 4) * 4)
    d_col.upload(np.arange(n, dtype=np.uint32))
    d_val = synth.DeviceBuffer((n + 4) * 4)
    d_val.upload(np.full(n, 0.25, np.float32))
    shift = sm.SparseMatCRS.from_device_parts(n, n, n, d_off.ptr, d_col.ptr, d_val.ptr, np.float32, keep=(d_off, d_col, d_val))
    ms, best, _ = timed(lambda: a + shift, args.reps)
    report("(b) A + 0.25 I, %d^3 f32" % g, ms, best, 2 * ab + crs_bytes(shift), route())
    del a, shift

    # (c) C3 shape plus its transpose
    p = synth.crs_powerlaw(0x5EED0001, args.c3_rows, args.c3_rows, np.float64)
    pb = crs_bytes(p)
    ms, best, pt = timed(lambda: p.transpose(), args.reps)
    report("(c) transpose(P) yardstick, C3 %d rows f64" % args.c3_rows, ms, best, 2 * pb, sm.SparseMatCRS.last_transpose_route())
    ms, best, s = timed(lambda: p + pt, args.reps)
    report("(c) P + P^T, C3 %d rows f64" % args.c3_rows, ms, best, 2 * pb + crs_bytes(s), route(),
           {"nnz_P": p.n_non_zero_entries(), "nnz_sum": s.n_non_zero_entries()})


if __name__ == "__main__":
    main()
