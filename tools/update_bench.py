#!/usr/bin/env python3
"""Times batched element access of SparseMatCRS on one GPU (development aid, not the contract bench): smh_crs_apply and
smh_crs_get_many_dev of csrc/matupdate.hip on the shapes of the issue that introduced them, and the reusable update plan of
csrc/matplan.hip beside them.

  (a) re-assembly: the 128^3-cell trilinear hexahedral mesh (134 M add_to operations, 2.1 M rows, 57 M entries, f32) applied to
      its own assembled matrix (values-only route), next to smh_crs_assemble_dev of the same stream in the same run; then the
      update plan of the same stream: its create, and its execute with from_zero 0 and 1 on the same device arrays, each
      repetition timing apply_dev, execute(0) and execute(1) in turn;
  (b) the 512^3 7-point Laplacian f32: a diagonal-shift stream (values only) next to `A += 0.25 I`, and a stream adding one
      new entry per row (general route; each repetition starts from a clone made outside the timed region);
  (c) get_many_dev of 10 M queries of existing entries on the 512^3 Laplacian and on the C3 shape (f64 power law 1-2048,
      10 M rows): queries per second;
  (d) skew, reported only: 1 M add_to onto ONE entry of a small Laplacian, plan execute next to apply_dev.

Each call is synchronous; HIP events on the null stream bracket it, so a figure is the whole call.  Algorithmic bytes:
(a) / (b) the operation arrays read once, the matrix's offsets and columns read once, its values read and written once (the
general route: the result's arrays written once as well); (c) the query arrays read, the answers written, and the offsets
plus one column per query read; a plan execute: the values read once, the plan's arrays read once, the targeted matrix
values read and written once (from_zero: written only).

    python tools/update_bench.py [--grid 128] [--lap 512] [--c3-rows 10000000] [--reps 3] [--cases abcd]
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


def timed(fn, reps, setup=None):
    """median and best ms of `fn` (setup() runs before each repetition, outside the events; its result is passed on)"""
    e0, e1 = C.c_void_p(), C.c_void_p()
    check(lib().smh_event_create(C.byref(e0)))
    check(lib().smh_event_create(C.byref(e1)))
    ts, keep = [], None
    try:
        for _ in range(reps):
            keep = None
            arg = setup() if setup else None
            check(lib().smh_device_synchronize())
            check(lib().smh_event_record(e0, None))
            keep = fn(arg) if setup else fn()
            check(lib().smh_event_record(e1, None))
            ms = C.c_float()
            check(lib().smh_event_elapsed_ms(e0, e1, C.byref(ms)))
            ts.append(ms.value)
    finally:
        lib().smh_event_destroy(e0)
        lib().smh_event_destroy(e1)
    ts.sort()
    return ts[len(ts) // 2], ts[0], keep


def timed_in_turn(fns, reps):
    """[(median ms, best ms)] of every fn, each repetition timing them one after the other (same events, same bracketing)"""
    e0, e1 = C.c_void_p(), C.c_void_p()
    check(lib().smh_event_create(C.byref(e0)))
    check(lib().smh_event_create(C.byref(e1)))
    ts = [[] for _ in fns]
    try:
        for _ in range(reps):
            for k, fn in enumerate(fns):
                check(lib().smh_device_synchronize())
                check(lib().smh_event_record(e0, None))
                fn()
                check(lib().smh_event_record(e1, None))
                ms = C.c_float()
                check(lib().smh_event_elapsed_ms(e0, e1, C.byref(ms)))
                ts[k].append(ms.value)
    finally:
        lib().smh_event_destroy(e0)
        lib().smh_event_destroy(e1)
    return [(sorted(t)[len(t) // 2], min(t)) for t in ts]


def plan_bytes(st, vs, from_zero):
    """algorithmic bytes of one execute: values once, plan arrays once, targeted values read and written (from_zero: written)"""
    return vs * st["n_live_ops"] + st["device_bytes"] + (1 if from_zero else 2) * vs * st["n_targets"]


def plan_cases(name, m, n_ops, d, reps, ms_asm=None):
    """apply_dev, plan execute(from_zero=0) and execute(from_zero=1) of one stream on m, in turn; plan create beside them"""
    route = sm.SparseMatCRS.last_apply_route
    ms_c, best_c, plan = timed(lambda: m.update_plan_dev(n_ops, d[0].ptr, d[1].ptr), max(1, reps - 1))
    st = plan.stats()
    report("%s plan create" % name, ms_c, best_c, 8 * n_ops + crs_bytes(m) + st["device_bytes"], "plan_create", st)
    (ms_a, best_a), (ms_0, best_0), (ms_1, best_1) = timed_in_turn(
        [lambda: m.apply_dev(n_ops, d[0].ptr, d[1].ptr, d[2].ptr), lambda: plan.execute_dev(d[2].ptr, False), lambda: plan.execute_dev(d[2].ptr, True)], reps)
    extra = {"ratio_to_assemble": round(ms_a / ms_asm, 3)} if ms_asm else {}
    report("%s apply_dev" % name, ms_a, best_a, 12 * n_ops + crs_bytes(m) + 4 * m.n_non_zero_entries(), route(), extra)
    for fz, ms, best in ((0, ms_0, best_0), (1, ms_1, best_1)):
        extra = {"ratio_to_apply": round(ms / ms_a, 3)}
        if ms_asm:
            extra["ratio_to_assemble"] = round(ms / ms_asm, 3)
        report("%s plan execute from_zero=%d" % (name, fz), ms, best, plan_bytes(st, m.dtype.itemsize, fz), "plan_execute", extra)


def report(name, ms, best, nbytes, route, extra=None):
    line = {"case": name, "route": route, "ms": round(ms, 3), "best_ms": round(best, 3), "algorithmic_GB": round(nbytes / 1e9, 3),
            "GB_per_s": round(nbytes / 1e6 / ms, 1), "fraction_of_8TB_s": round(nbytes / 1e6 / ms / PEAK_GB_S, 3)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)


def dev_array(a):
    a = np.ascontiguousarray(a)
    buf = synth.DeviceBuffer(a.nbytes + 16)
    buf.upload(a)
    return buf


def hex_stream(g, dtype, rng):
    nodes = np.arange((g + 1) ** 3, dtype=np.uint32).reshape(g + 1, g + 1, g + 1)
    corners = np.stack([nodes[dx:g + dx, dy:g + dy, dz:g + dz].ravel()
                        for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)], axis=1)
    rows = np.repeat(corners, 8, axis=1).ravel()
    cols = np.tile(corners, (1, 8)).ravel()
    vals = rng.uniform(-1, 1, len(rows)).astype(dtype)
    return rows, cols, vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--lap", type=int, default=512)
    ap.add_argument("--c3-rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="abcd", help="which of the cases (a) .. (d) to run ((b) and (c) share their matrix and run together)")
    args = ap.parse_args()
    n_dev = C.c_int()
    check(lib().smh_device_count(C.byref(n_dev)))
    assert n_dev.value > 0, "needs a HIP device"
    rng = np.random.default_rng(1)
    if "a" in args.cases:
        case_a(args, rng)
    if "b" in args.cases or "c" in args.cases:
        case_bc(args, rng)
    if "d" in args.cases:
        case_d(args)


def case_a(args, rng):
    route = sm.SparseMatCRS.last_apply_route
    # (a) re-assembly of the hexahedral mesh
    rows, cols, vals = hex_stream(args.grid, np.float32, rng)
    n_ops = len(vals)
    d = [dev_array(rows), dev_array(cols), dev_array(vals)]
    del rows, cols, vals
    ms_asm, best, m = timed(lambda: sm.SparseMatCRS.from_device_triplets(n_ops, d[0].ptr, d[1].ptr, d[2].ptr, np.float32), args.reps)
    report("(a) assemble_dev yardstick, %d^3 cells f32" % args.grid, ms_asm, best, 12 * n_ops + crs_bytes(m), "assemble",
           {"n_ops": n_ops, "n_rows": m.n_rows(), "nnz": m.n_non_zero_entries()})
    ms, best, _ = timed(lambda: m.apply_dev(n_ops, d[0].ptr, d[1].ptr, d[2].ptr), args.reps)
    report("(a) re-assembly apply_dev, %d^3 cells f32" % args.grid, ms, best, 12 * n_ops + crs_bytes(m) + 4 * m.n_non_zero_entries(), route(),
           {"ratio_to_assemble": round(ms / ms_asm, 3)})
    plan_cases("(a) in turn, %d^3 cells f32:" % args.grid, m, n_ops, d, args.reps, ms_asm)


def case_d(args):
    # (d) skew: every operation on one entry
    g, n_ops = 16, 1_000_000
    a = synth.crs_laplace3d(g, g, g, np.float32)
    off, col, _ = a.raw_parts()
    i = a.n_rows() // 2
    d = [dev_array(np.full(n_ops, i, np.uint32)), dev_array(np.full(n_ops, col[off[i] + 1], np.uint32)),
         dev_array(np.random.default_rng(2).uniform(-1, 1, n_ops).astype(np.float32))]
    plan_cases("(d) %d add_to onto one entry, %d^3 Laplacian f32:" % (n_ops, g), a, n_ops, d, args.reps)


def case_bc(args, rng):
    route = sm.SparseMatCRS.last_apply_route
    # (b) the Laplacian: diagonal shift vs A += 0.25 I, and one new entry per row
    g = args.lap
    a = synth.crs_laplace3d(g, g, g, np.float32)
    n = a.n_rows()
    ab = crs_bytes(a)
    iota = dev_array(np.arange(n + 1, dtype=np.uint32))
    quarter = dev_array(np.full(n, 0.25, np.float32))
    shift = sm.SparseMatCRS.from_device_parts(n, n, n, iota.ptr, iota.ptr, quarter.ptr, np.float32, keep=(iota, quarter))
    ms, best, _ = timed(lambda: a.add(shift), args.reps)
    report("(b) A += 0.25 I, %d^3 f32" % g, ms, best, 2 * ab + crs_bytes(shift) + 4 * n, sm.SparseMatCRS.last_add_route())
    ms, best, _ = timed(lambda: a.apply_dev(n, iota.ptr, iota.ptr, quarter.ptr), args.reps)
    report("(b) apply of the diagonal shift, %d^3 f32" % g, ms, best, 12 * n + ab + 4 * n, route())
    far = dev_array(((np.arange(n, dtype=np.int64) + n // 2) % n).astype(np.uint32))
    ms, best, r = timed(lambda c: (c.apply_dev(n, iota.ptr, far.ptr, quarter.ptr), c)[1], max(1, args.reps - 1), setup=lambda: a.clone())
    report("(b) apply of one new entry per row, %d^3 f32" % g, ms, best, 12 * n + ab + crs_bytes(r), route(),
           {"nnz_before": a.n_non_zero_entries(), "nnz_after": r.n_non_zero_entries()})
    del r, far

    # (c) get_many_dev
    q = args.queries
    qi = rng.integers(0, n, q)
    step = np.array([0, 1, -1, g, -g, g * g, -g * g])[rng.integers(0, 7, q)]
    qj = qi + step
    qj = np.where((qj < 0) | (qj >= n), qi, qj)
    dq = [dev_array(qi.astype(np.uint32)), dev_array(qj.astype(np.uint32)), synth.DeviceBuffer(q * 8 + 16)]
    ms, best, _ = timed(lambda: a.get_many_dev(q, dq[0].ptr, dq[1].ptr, dq[2].ptr), args.reps)
    report("(c) get_many_dev, %d^3 Laplacian f32" % g, ms, best, q * (8 + 4 + 8 + 4), "lookup", {"queries_per_s": round(q / ms * 1e3)})
    del a, shift, dq
    p = synth.crs_powerlaw(0x5EED0001, args.c3_rows, args.c3_rows, np.float64)
    off, col, _ = p.raw_parts()
    lens = np.diff(off.astype(np.int64))
    nz_rows = np.flatnonzero(lens)
    qi = nz_rows[rng.integers(0, len(nz_rows), q)]
    qk = off[qi].astype(np.int64) + rng.integers(0, 1 << 62, q) % lens[qi]
    qj = col[qk]
    del off, col
    dq = [dev_array(qi.astype(np.uint32)), dev_array(qj.astype(np.uint32)), synth.DeviceBuffer(q * 8 + 16)]
    ms, best, _ = timed(lambda: p.get_many_dev(q, dq[0].ptr, dq[1].ptr, dq[2].ptr), args.reps)
    report("(c) get_many_dev, C3 %d rows f64" % args.c3_rows, ms, best, q * (8 + 8 + 8 + 4), "lookup",
           {"queries_per_s": round(q / ms * 1e3), "max_row_len": p.max_row_len()})


if __name__ == "__main__":
    main()
