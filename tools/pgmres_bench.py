#!/usr/bin/env python3
"""Ad-hoc timing of the right-preconditioned GMRES (smh_gmres_precond_solve_vec, an extension) on one GPU (development aid, not the
contract bench).

Shape: tools/bicgstab_bench.py's non-symmetric 7-point operator ("lap-nonsym"), in the natural ordering and in the multicolour one
(SparseMatCRS.color + permute_symmetric; b is permuted with it, so both orderings solve the same system).  That operator has
positive off-diagonal entries that outweigh its diagonal: it is indefinite, and no side reaches a tolerance on it (its bodies are
timed all the same).  --shape convdiff is the operator the solvers can be compared on to a tolerance: the 7-point Laplacian with
upwind convection, the three lower neighbours times 1 + c and 3 c added to the diagonal (c = 1: -2, 9, -1; zero row sums inside),
the 3-d sibling of the tests' convdiff2d.

To a tolerance (tol = --rtol * |b|, from x0 = 0): GMRES(30) unpreconditioned, with Jacobi, SGS and ILU(0), and BiCGSTAB.  All sides
alternate on one handle in one process; a warm-up round, then the median of --repeats rounds.  Per side: bodies, ms to tol (HIP
events around one synchronous solve on device-resident vectors: set-up and polls included), ms per body (their quotient), and the
true residual |b - A x| / |b| formed on the device in the working precision.  Beside them the one-off costs, wall clock around
synchronous calls: colouring + permutation, ilu0, and the two level schedules (the first trisolve_levels calls).

The Jacobi body against the unpreconditioned one at fixed work (tol 0): the difference quotient of a solve of one full cycle and
one of three, as tools/gmres_bench.py does, next to the byte model's ratio.  A GMRES(m) body averaged over a cycle moves, beside its
product, (2 m + 11) + (m + 7) / m n-vectors unpreconditioned and (2 m + 12) + (m + 9) / m with Jacobi: one read of d in
every normalisation, one in the cycle end's sweep, one in the restart's v_0."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import synth  # noqa: E402
from sparsemat_amd._lib import check, lib  # noqa: E402
from cg_many_bench import Events  # noqa: E402
import bicgstab_bench  # noqa: E402  (the operator)
import mvp_many_bench  # noqa: E402  (the product's byte model)

RESTART = 30
med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731


def wall(work):
    check(lib().smh_device_synchronize())
    t0 = time.perf_counter()
    out = work()
    check(lib().smh_device_synchronize())
    return out, (time.perf_counter() - t0) * 1e3


def to_tol(a, factor, b_host, tol, iter_max, dtype, args, ev, label):
    n = a.n_rows()
    b = sm.DenseVec.from_vec(b_host)
    norm_b = float(np.linalg.norm(b_host.astype(np.float64)))
    sides = [("GMRES(30)", lambda: sm.GMRES(tol, iter_max, RESTART), None),
             ("GMRES(30) + Jacobi", lambda: sm.GMRES(tol, iter_max, RESTART, precond="jacobi"), None),
             ("GMRES(30) + SGS", lambda: sm.GMRES(tol, iter_max, RESTART, precond="sgs"), None),
             ("GMRES(30) + ILU(0)", lambda: sm.GMRES(tol, iter_max, RESTART, precond="ilu"), factor),
             ("BiCGSTAB", lambda: sm.BiCGStab(tol, iter_max), None)]
    ms, info = {name: [] for name, _, _ in sides}, {}
    for rep in range(args.repeats + 1):  # (the first round warms every side up and is not counted)
        for name, make, f in sides:
            x = sm.DenseVec.zeros(n, dtype)
            s = make()
            t = ev.ms((lambda: s.solve(a, b, x, factor=f)) if f is not None else (lambda: s.solve(a, b, x)))
            if rep:
                ms[name].append(t)
            xh = x.to_numpy()
            true = float(np.linalg.norm((b_host - a.mvp(xh)).astype(np.float64))) / norm_b
            info[name] = (s.iterations, getattr(s, "breakdown", 0), true)
    for name, _, _ in sides:
        bodies, brk, true = info[name]
        t = ms[name]
        print("    %-10s %-20s %5d bodies%s | %9.2f ms to tol (%.2f .. %.2f) | %7.3f ms per body | true residual %.2e |b|" % (
            label, name, bodies, " (breakdown %d)" % brk if brk else "", med(t), min(t), max(t), med(t) / max(bodies, 1), true), flush=True)


def jacobi_body(a, b_host, dtype, args, ev):
    n, vs = a.n_rows(), np.dtype(dtype).itemsize
    b = sm.DenseVec.from_vec(b_host)
    shape = {"entries_per_row": 7, "single_offset_bytes": 1, "single_reads_no_values": False}
    product = mvp_many_bench.model_bytes(shape, vs, 1)[1]  # bytes per row of one product

    def per_body(precond):
        t = []
        for bodies in (RESTART, 3 * RESTART):
            x = sm.DenseVec.zeros(n, dtype)
            s = sm.GMRES(0.0, bodies, RESTART, precond=precond)
            t.append(ev.ms(lambda: s.solve(a, b, x)))
            assert s.iterations == bodies, (s.iterations, bodies, s.breakdown)
        return (t[1] - t[0]) / (2 * RESTART)

    plain, jac = [], []
    for rep in range(args.repeats + 1):
        p, j = per_body(None), per_body("jacobi")
        if rep:
            plain.append(p)
            jac.append(j)
    m = RESTART
    model = (product + (2 * m + 12 + (m + 9) / m) * vs) / (product + (2 * m + 11 + (m + 7) / m) * vs)
    ratio = [j / p for j, p in zip(jac, plain)]
    print("    body at fixed work: GMRES(30) %.3f ms (%.3f .. %.3f), + Jacobi %.3f ms (%.3f .. %.3f): ratio %.4f (%.4f .. %.4f) against "
          "the byte model's %.4f" % (med(plain), min(plain), max(plain), med(jac), min(jac), max(jac), med(ratio), min(ratio), max(ratio), model),
          flush=True)


def build(args, dtype):
    if args.shape == "lap-nonsym":
        return bicgstab_bench.build("lap-nonsym", args.grid, dtype)
    g, c = args.grid, 1.0
    m = synth.crs_laplace3d(g, g, g, dtype)
    off, col, val = m.raw_parts()
    rows = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off.astype(np.int64)))
    m.update_values(np.where(col < rows, val * (1 + c), np.where(col == rows, val + 3 * c, val)).astype(dtype))
    return m


def run(dtype, args, ev):
    a = build(args, dtype)
    n = a.n_rows()
    a.sort_rows()  # (ilu0 needs ascending rows; a no-op on this operator)
    a.prepare("auto")
    bd = sm.DenseVec.zeros(n, dtype)
    synth.gen_x(synth.SEED_X, n, dtype, ptr=bd.data_ptr())
    b = bd.to_numpy()
    tol = args.rtol[dtype] * float(np.linalg.norm(b.astype(np.float64)))
    print("%s %d^3 %s auto=%s: tol = %.1e |b| = %.3e" % (args.shape, args.grid, np.dtype(dtype).name, a.resolved_variant(), args.rtol[dtype], tol), flush=True)
    jacobi_body(a, b, dtype, args, ev)
    (perm, stats), t_color = wall(lambda: a.color())
    c, t_perm = wall(lambda: a.permute_symmetric(perm))
    c.sort_rows()
    c.prepare("auto")
    for label, mat, rhs in (("natural", a, b), ("multicolour", c, b[perm.astype(np.int64)])):
        (f, zp), t_ilu = wall(lambda: mat.ilu0())
        lv, t_sched = {}, 0.0
        for h, who in ((mat, "matrix"), (f, "factor")):
            for uplo in ("lower", "upper"):
                lv[who, uplo], t = wall(lambda: h.trisolve_levels(uplo))
                t_sched += t
        print("    %-10s ilu0 %.1f ms (zero pivot %s) | four level schedules %.1f ms | levels %d, launches per solve %d%s" % (
            label, t_ilu, zp, t_sched, lv["matrix", "lower"]["n_levels"], lv["matrix", "lower"]["n_launches"],
            " | colouring %.1f ms (%d colours), permutation %.1f ms" % (t_color, stats["n_colors"], t_perm) if label == "multicolour" else ""), flush=True)
        to_tol(mat, f, rhs, tol, args.iter_max, dtype, args, ev, label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="lap-nonsym", choices=["lap-nonsym", "convdiff"])
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--rtol32", type=float, default=1e-4)
    ap.add_argument("--rtol64", type=float, default=1e-8)
    ap.add_argument("--iter-max", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    args.rtol = {np.float32: args.rtol32, np.float64: args.rtol64}
    ev = Events()
    for dt in args.dtypes.split(","):
        run({"f32": np.float32, "f64": np.float64}[dt], args, ev)
        check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
