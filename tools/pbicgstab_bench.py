#!/usr/bin/env python3
"""Ad-hoc timing of the right-preconditioned BiCGSTAB (smh_bicgstab_precond_solve_vec, an extension) on one GPU (development aid,
not the contract bench).

Shapes: tools/pgmres_bench.py's --shape convdiff (the 7-point Laplacian with upwind convection, -2 / 9 / -1 at c = 1; --convection
sets c), in the natural ordering and in the multicolour one (SparseMatCRS.color + permute_symmetric; b is permuted with it, so both
orderings solve the same system); and "convdiff-scaled": that operator with row i scaled by 2^k_i, k uniform in -5 .. 5 (exact), the
right-hand side scaled with it -- a system where Jacobi should decide the body count.

To a tolerance (tol = --rtol * |b|, from x0 = 0): BiCGSTAB unpreconditioned, with Jacobi, SGS and ILU(0), and ILU-GMRES(30) as the
yardstick.  All sides alternate on one handle in one process; a warm-up round, then the median of --repeats rounds with the spread.
Per side: bodies, ms to tol (HIP events around one synchronous solve on device-resident vectors: set-up and polls included), ms per
body (their quotient), and the true residual |b - A x| / |b| (the device's product of x in the working precision; the difference
and the norm in f64 on the host).

At fixed work (tol 0; the difference quotient of solves of --bodies and 3 x --bodies bodies, as tools/bicgstab_bench.py): the
unpreconditioned body through smh_bicgstab_solve_vec, the same body through smh_bicgstab_precond_solve_vec's SMH_PRECOND_NONE, and the
Jacobi body, next to the byte model's ratio: a body moves two products + 18 n values unpreconditioned and two products + 23 n with
Jacobi.  The first figure is the one to hold beside tools/bicgstab_bench.py run on the parent commit in the same
session: the unpreconditioned (kPcNone) instantiation must cost nothing."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import synth  # noqa: E402
from sparsemat_amd._lib import SMH_PRECOND_NONE, check, lib  # noqa: E402
from cg_many_bench import Events  # noqa: E402
import mvp_many_bench  # noqa: E402  (the product's byte model)
from pgmres_bench import RESTART, med, wall  # noqa: E402

PLAIN_VALUES, JACOBI_VALUES = 18, 23  # per body beside the two products


def spread(v):
    return "%.2f .. %.2f" % (min(v), max(v))


def to_tol(a, factor, b_host, tol, iter_max, dtype, args, ev, label):
    n = a.n_rows()
    b = sm.DenseVec.from_vec(b_host)
    b64 = b_host.astype(np.float64)
    norm_b = float(np.linalg.norm(b64))
    sides = [("BiCGSTAB", lambda: sm.BiCGStab(tol, iter_max), None),
             ("BiCGSTAB + Jacobi", lambda: sm.BiCGStab(tol, iter_max, precond="jacobi"), None),
             ("BiCGSTAB + SGS", lambda: sm.BiCGStab(tol, iter_max, precond="sgs"), None),
             ("BiCGSTAB + ILU(0)", lambda: sm.BiCGStab(tol, iter_max, precond="ilu"), factor),
             ("GMRES(30) + ILU(0)", lambda: sm.GMRES(tol, iter_max, RESTART, precond="ilu"), factor)]
    if label in args.skip_tri:
        sides = [s for s in sides if s[0] in ("BiCGSTAB", "BiCGSTAB + Jacobi")]
    ms, info = {name: [] for name, _, _ in sides}, {}
    for rep in range(args.repeats + 1):  # (the first round warms every side up and is not counted)
        for name, make, f in sides:
            x = sm.DenseVec.zeros(n, dtype)
            s = make()
            t = ev.ms((lambda: s.solve(a, b, x, factor=f)) if f is not None else (lambda: s.solve(a, b, x)))
            if rep:
                ms[name].append(t)
            if rep == args.repeats:
                true = float(np.linalg.norm(b64 - a.mvp(x.to_numpy()).astype(np.float64))) / norm_b
                info[name] = (s.iterations, getattr(s, "breakdown", 0), true)
    for name, _, _ in sides:
        bodies, brk, true = info[name]
        t = ms[name]
        print("    %-11s %-20s %5d bodies%s | %9.2f ms to tol (%s) | %7.3f ms per body | true residual %.2e |b|" % (
            label, name, bodies, " (breakdown %d)" % brk if brk else "", med(t), spread(t), med(t) / max(bodies, 1), true), flush=True)


def fixed_work(a, b_host, dtype, args, ev):
    n, vs = a.n_rows(), np.dtype(dtype).itemsize
    b = sm.DenseVec.from_vec(b_host)
    shape = {"entries_per_row": 7, "single_offset_bytes": 1, "single_reads_no_values": False}
    product = mvp_many_bench.model_bytes(shape, vs, 1)[1]  # bytes per row of one product
    lo, hi = args.bodies, 3 * args.bodies

    class ThroughNone(sm.BiCGStab):
        """the unpreconditioned solve entered through smh_bicgstab_precond_solve_vec(SMH_PRECOND_NONE)"""

        def solve(self, mat, b, x):
            brk = C.c_int()
            self._solve(lib().smh_bicgstab_precond_solve_vec, None, mat, b, x, handles=(SMH_PRECOND_NONE, None), extra_out=(brk,))
            self.breakdown = brk.value

    def per_body(make):
        t = []
        for bodies in (lo, hi):
            x = sm.DenseVec.zeros(n, dtype)
            s = make(bodies)
            t.append(ev.ms(lambda: s.solve(a, b, x)))
            assert s.iterations == bodies, (s.iterations, bodies, s.breakdown)
        return (t[1] - t[0]) / (hi - lo)

    makers = [("plain", lambda k: sm.BiCGStab(0.0, k)), ("none", lambda k: ThroughNone(0.0, k)), ("jacobi", lambda k: sm.BiCGStab(0.0, k, precond="jacobi"))]
    t = {name: [] for name, _ in makers}
    for rep in range(args.repeats + 1):
        for name, make in makers:
            v = per_body(make)
            if rep:
                t[name].append(v)
    model = (2 * product + JACOBI_VALUES * vs) / (2 * product + PLAIN_VALUES * vs)
    ratio = [j / p for j, p in zip(t["jacobi"], t["plain"])]
    print("    body at fixed work (%d and %d bodies): smh_bicgstab_solve_vec %.4f ms (%.4f .. %.4f) | SMH_PRECOND_NONE %.4f ms (%.4f .. %.4f) | "
          "+ Jacobi %.4f ms (%.4f .. %.4f): ratio %.4f (%.4f .. %.4f) against the byte model's %.4f (%d against %d B per row)" % (
              lo, hi, med(t["plain"]), min(t["plain"]), max(t["plain"]), med(t["none"]), min(t["none"]), max(t["none"]),
              med(t["jacobi"]), min(t["jacobi"]), max(t["jacobi"]), med(ratio), min(ratio), max(ratio), model,
              2 * product + JACOBI_VALUES * vs, 2 * product + PLAIN_VALUES * vs), flush=True)


def build(args, dtype, scaled):
    """pgmres_bench's convdiff with c = --convection; scaled: row i times 2^k_i (returns the handle and the row scales, or None)"""
    g, c = args.grid, args.convection
    m = synth.crs_laplace3d(g, g, g, dtype)
    off, col, val = m.raw_parts()
    counts = np.diff(off.astype(np.int64))
    rows = np.repeat(np.arange(len(off) - 1, dtype=np.int64), counts)
    val = np.where(col < rows, val * (1 + c), np.where(col == rows, val + 3 * c, val)).astype(dtype)
    scale = None
    if scaled:
        scale = (2.0 ** np.random.default_rng(7).integers(-5, 6, len(off) - 1)).astype(dtype)
        val = val * np.repeat(scale, counts)
    m.update_values(val)
    return m, scale


def run(shape, dtype, args, ev):
    a, scale = build(args, dtype, shape == "convdiff-scaled")
    n = a.n_rows()
    a.sort_rows()  # (ilu0 needs ascending rows; a no-op on this operator)
    a.prepare("auto")
    bd = sm.DenseVec.zeros(n, dtype)
    synth.gen_x(synth.SEED_X, n, dtype, ptr=bd.data_ptr())
    b = bd.to_numpy()
    if scale is not None:
        b = b * scale
    tol = args.rtol[dtype] * float(np.linalg.norm(b.astype(np.float64)))
    print("%s (c = %g) %d^3 %s auto=%s: tol = %.1e |b| = %.3e" % (shape, args.convection, args.grid, np.dtype(dtype).name, a.resolved_variant(),
                                                                  args.rtol[dtype], tol), flush=True)
    if shape == "convdiff":
        fixed_work(a, b, dtype, args, ev)
    (perm, stats), t_color = wall(lambda: a.color())
    c, t_perm = wall(lambda: a.permute_symmetric(perm))
    c.sort_rows()
    c.prepare("auto")
    for label, mat, rhs in (("natural", a, b), ("multicolour", c, b[perm.astype(np.int64)])):
        f = None
        if label not in args.skip_tri:
            (f, zp), t_ilu = wall(lambda: mat.ilu0())
            lv = mat.trisolve_levels("lower")
            print("    %-11s ilu0 %.1f ms (zero pivot %s) | levels %d, launches per solve %d%s" % (
                label, t_ilu, zp, lv["n_levels"], lv["n_launches"],
                " | colouring %.1f ms (%d colours), permutation %.1f ms" % (t_color, stats["n_colors"], t_perm) if label == "multicolour" else ""), flush=True)
        to_tol(mat, f, rhs, tol, args.iter_max, dtype, args, ev, label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="convdiff,convdiff-scaled")
    ap.add_argument("--convection", type=float, default=1.0, help="c: the lower neighbours times 1 + c, 3 c added to the diagonal")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--rtol32", type=float, default=1e-4)
    ap.add_argument("--rtol64", type=float, default=1e-6)
    ap.add_argument("--iter-max", type=int, default=3000)
    ap.add_argument("--bodies", type=int, default=20, help="fixed work: the shorter solve; the longer one runs three times as many")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-tri", default="", help="orderings (natural,multicolour) on which the SGS / ILU(0) sides are left out")
    args = ap.parse_args()
    args.rtol = {np.float32: args.rtol32, np.float64: args.rtol64}
    args.skip_tri = [s for s in args.skip_tri.split(",") if s]
    ev = Events()
    for shape in args.shapes.split(","):
        for dt in args.dtypes.split(","):
            run(shape, {"f32": np.float32, "f64": np.float64}[dt], args, ev)
            check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
