#!/usr/bin/env python3
"""Ad-hoc timing of the multicolour ordering (smh_crs_color, an extension) and of what it buys the level-scheduled triangular solves
and SGS-PCG, on one GPU (development aid, not the contract bench).  The operators, the red-black permutation and the timing
helpers are tools/sgs_bench.py's.  The sides of every comparison alternate in one process; medians with min .. max over
`--repeats` pairings after a warm-up pairing.

Per operator (the 7-point operator on g3^3 and the 5-point operator on g2^2 with non-constant coefficients, f32 and f64, in the
natural ordering): the wall time of `color` with n_colors, n_rounds and color_counts beside `rcm` on the same handle; the wall
time of permute_symmetric by the colouring.  Then on each of the natural, the multicolour and the red-black ordering of the same
system (the right-hand side permuted along): the schedule's build time with its level and launch counts; a LOWER + UPPER solve
pair; the AUTO product's kernel and time; bodies and wall time to tolerance of CG, Jacobi-PCG and SGS-PCG from x0 = 0."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sgs_bench import build, med, red_black_perm, spread, wall_ms  # noqa: E402
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import _lib  # noqa: E402
from sparsemat_amd._lib import check, lib  # noqa: E402


def order(label, a, dtype, args):
    """color beside rcm on the same handle, then permute_symmetric by the colouring; returns the permutation"""
    t_color, t_rcm, t_perm = [], [], []
    out = {}
    for rep in range(args.repeats + 1):
        p = wall_ms(lambda: out.__setitem__("color", a.color(args.seed)))
        q = wall_ms(lambda: out.__setitem__("rcm", a.rcm()))
        r = wall_ms(lambda: out.__setitem__("b", a.permute_symmetric(out["color"][0])))
        out.pop("b")
        if rep:
            t_color.append(p)
            t_rcm.append(q)
            t_perm.append(r)
    perm, st = out["color"]
    _, rst = out["rcm"]
    # the same two on device arrays (the _dev forms): no copy of 2 n words to the host, no bincount there
    import ctypes as C
    n = a.n_rows()
    dc, dp = sm.DenseVec.zeros(n, np.float32), sm.DenseVec.zeros(n, np.float32)
    d_color, d_rcm = [], []
    for rep in range(args.repeats + 1):
        p = wall_ms(lambda: check(lib().smh_crs_color_dev(a._h, args.seed, C.c_void_p(dc.data_ptr()), C.c_void_p(dp.data_ptr()), None, None)))
        q = wall_ms(lambda: check(lib().smh_crs_rcm_dev(a._h, C.c_void_p(dp.data_ptr()), None, None)))
        if rep:
            d_color.append(p)
            d_rcm.append(q)
    del dc, dp
    print("%s: on device arrays: color %s ms | rcm %s ms | ratio rcm / color %.1f" % (label, spread(d_color), spread(d_rcm), med(d_rcm) / med(d_color)), flush=True)
    print("%s: color %s ms (%d colours, %d rounds, color_counts %s) | rcm %s ms (%d levels) | ratio rcm / color %.1f | permute_symmetric %s ms" % (
        label, spread(t_color), st["n_colors"], st["n_rounds"], st["color_counts"].tolist(), spread(t_rcm), rst["n_levels"], med(t_rcm) / med(t_color),
        spread(t_perm)), flush=True)
    return perm


def run(label, a, b_host, dtype, args):
    n = a.n_rows()
    t_build = wall_ms(lambda: (a.trisolve_levels("lower"), a.trisolve_levels("upper")))
    lo, up = a.trisolve_levels("lower"), a.trisolve_levels("upper")
    a.prepare("auto")
    print("%s: auto=%s | schedule build (both triangles) %.1f ms | levels %d / %d | launches per solve %d / %d" % (
        label, a.resolved_variant(), t_build, lo["n_levels"], up["n_levels"], lo["n_launches"], up["n_launches"]), flush=True)
    b = sm.DenseVec.from_vec(b_host)
    w, y = sm.DenseVec.zeros(n, dtype), sm.DenseVec.zeros(n, dtype)
    L = lib()

    def pair():
        check(L.smh_crs_trisolve_vec(a._h, _lib.SMH_TRI_LOWER, _lib.SMH_DIAG_NON_UNIT, b._h, w._h))
        check(L.smh_crs_trisolve_vec(a._h, _lib.SMH_TRI_UPPER, _lib.SMH_DIAG_NON_UNIT, w._h, w._h))

    def product():
        a.mvp_dev(b.data_ptr(), n, y.data_ptr(), "auto")

    t_pair, t_prod = [], []
    for rep in range(args.repeats + 1):
        p, q = wall_ms(pair), wall_ms(product)
        if rep:
            t_pair.append(p)
            t_prod.append(q)
    print("%s: LOWER + UPPER solve pair %s ms | one AUTO product %s ms | ratio %.1f" % (label, spread(t_pair), spread(t_prod), med(t_pair) / med(t_prod)),
          flush=True)
    norm_b = float(np.sqrt(np.sum(b_host.astype(np.float64) ** 2)))
    tol = (args.tol32 if dtype == np.float32 else args.tol64) * norm_b
    times = {}
    solvers = (("CG", sm.ConjugateGradient), ("Jacobi-PCG", sm.JacobiConjugateGradient), ("SGS-PCG", sm.SGSConjugateGradient))
    for rep in range(args.repeats + 1):  # (the three solvers alternate)
        for what, cls in solvers:
            x = np.zeros(n, dtype)
            s = cls(tol, args.iter_max)
            t = wall_ms(lambda: s.solve(a, b_host, x))
            if rep:
                times.setdefault(what, ([], s.iterations, s.r_norm_squared))[0].append(t)
    out = ["%s %d bodies %s ms%s" % (what, times[what][1], spread(times[what][0]), "" if np.sqrt(times[what][2]) < tol else " (NOT converged)")
           for what, _ in solvers]
    print("%s: to |r| < %.3g (%.0e |b|): %s" % (label, tol, tol / norm_b, " | ".join(out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g3", type=int, default=256, help="the 7-point operator's grid (g3^3)")
    ap.add_argument("--g2", type=int, default=1024, help="the 5-point operator's grid (g2^2)")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iter-max", type=int, default=5000)
    ap.add_argument("--tol32", type=float, default=1e-4, help="relative to |b|")
    ap.add_argument("--tol64", type=float, default=1e-8)
    args = ap.parse_args()
    shapes = ([("lap3d-%d" % args.g3, (args.g3, args.g3, args.g3))] if args.g3 else []) + ([("lap2d-%d" % args.g2, (args.g2, args.g2, 1))] if args.g2 else [])
    for name, dims in shapes:
        for dt in args.dtypes.split(","):
            dtype = {"f32": np.float32, "f64": np.float64}[dt]
            natural = build(dims, dtype)
            n = natural.n_rows()
            label = "%s %s" % (name, np.dtype(dtype).name)
            print("%s: n %d nnz %d" % (label, n, natural.n_non_zero_entries()), flush=True)
            perm = order(label, natural, dtype, args)
            b_host = np.random.default_rng(5).uniform(-1.0, 1.0, n).astype(dtype)
            for ordering, p in (("natural", None), ("multicolour", perm), ("red-black", red_black_perm(dims))):
                a = natural if p is None else natural.permute_symmetric(p)
                run("%s %s" % (label, ordering), a, b_host if p is None else b_host[p], dtype, args)
                del a
            del natural
            check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
