#!/usr/bin/env python3
"""Ad-hoc timing of the ILU(0) factorization and the ILU(0)-preconditioned CG (smh_crs_ilu0, smh_crs_ilu0_refactor,
smh_pcg_ilu_solve: extensions) on one GPU (development aid, not the contract bench).  The sides of every comparison alternate in
one process; medians with min .. max over `--repeats` rounds after a warm-up round.

Matrices, f32 and f64: tools/sgs_bench.py's 7-point operator on g3^3 and 5-point operator on g2^2, each in the natural ordering,
renumbered by the device multicolour ordering (color) and renumbered red-black (permute_symmetric, then sort_rows: ilu0 wants
every row's columns ascending).

Per matrix: a fresh ilu0 (clone, create-time inspection, the LOWER schedule's build and the factorization: wall), then in
alternation ilu0_refactor (pattern check, comparison and copy of the values, the factorization on the existing schedule) and one
LOWER unit-diagonal solve on the factor -- the same schedule and launch count --, and the LOWER schedule's build alone on a clone;
then wall time and bodies to tol for CG, Jacobi-PCG, SGS-PCG and ILU-PCG (the factor made before and passed in) from x0 = 0, host
vectors for all four, the four solvers alternating."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sgs_bench import build, med, red_black_perm, spread, wall_ms  # noqa: E402
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import _lib  # noqa: E402
from sparsemat_amd._lib import check, lib  # noqa: E402


def run(label, a, dtype, args):
    n = a.n_rows()
    name = "%s %s" % (label, np.dtype(dtype).name)
    a.prepare("auto")
    made = {}
    t_fresh = wall_ms(lambda: made.update(f=a.ilu0()))
    f, zero_pivot = made["f"]
    lv = f.trisolve_levels("lower")
    print("%s: n %d nnz %d auto=%s | levels %d | launches per factorization / LOWER solve %d (R = %d) | zero pivot %s | fresh ilu0 %.1f ms" % (
        name, n, a.n_non_zero_entries(), a.resolved_variant(), lv["n_levels"], lv["n_launches"], lv["small_level_rows"], zero_pivot, t_fresh), flush=True)
    rng = np.random.default_rng(5)
    b_host = rng.uniform(-1.0, 1.0, n).astype(dtype)
    b, w = sm.DenseVec.from_vec(b_host), sm.DenseVec.zeros(n, dtype)
    L = lib()
    t_ref, t_low, t_sched, t_new = [], [], [], []
    for rep in range(args.repeats + 1):
        p = wall_ms(lambda: f.ilu0_refactor(a))
        q = wall_ms(lambda: check(L.smh_crs_trisolve_vec(f._h, _lib.SMH_TRI_LOWER, _lib.SMH_DIAG_UNIT, b._h, w._h)))
        c = a.clone()
        s = wall_ms(lambda: c.trisolve_levels("lower"))
        del c
        r = wall_ms(lambda: a.ilu0())
        if rep:
            t_ref.append(p), t_low.append(q), t_sched.append(s), t_new.append(r)
    print("%s: ilu0_refactor %s ms | one LOWER solve %s ms | ratio %.1f | LOWER schedule build %s ms | fresh ilu0 %s ms" % (
        name, spread(t_ref), spread(t_low), med(t_ref) / med(t_low), spread(t_sched), spread(t_new)), flush=True)

    norm_b = float(np.sqrt(np.sum(b_host.astype(np.float64) ** 2)))
    tol = (args.tol32 if dtype == np.float32 else args.tol64) * norm_b
    solvers = (("CG", sm.ConjugateGradient, {}), ("Jacobi-PCG", sm.JacobiConjugateGradient, {}), ("SGS-PCG", sm.SGSConjugateGradient, {}),
               ("ILU-PCG", sm.ILUConjugateGradient, {"factor": f}))
    times = {what: [] for what, _, _ in solvers}
    result = {}
    for rep in range(args.solve_repeats + 1):
        for what, cls, kw in solvers:
            x = np.zeros(n, dtype)
            s = cls(tol, args.iter_max)
            t = wall_ms(lambda: s.solve(a, b_host, x, **kw))
            result[what] = (s.iterations, s.r_norm_squared)
            if rep:
                times[what].append(t)
    out = ["%s %d bodies %s ms%s" % (what, result[what][0], spread(times[what]),
                                     "" if np.sqrt(result[what][1]) < tol else " (NOT converged: |r| %.3g)" % np.sqrt(result[what][1]))
           for what, _, _ in solvers]
    print("%s: to |r| < %.3g (%.0e |b|): %s" % (name, tol, tol / norm_b, " | ".join(out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g3", type=int, default=256, help="the 7-point operator's grid (g3^3)")
    ap.add_argument("--g2", type=int, default=1024, help="the 5-point operator's grid (g2^2)")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--orderings", default="natural,color,red-black")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--iter-max", type=int, default=5000)
    ap.add_argument("--tol32", type=float, default=1e-4, help="relative to |b|")
    ap.add_argument("--tol64", type=float, default=1e-8)
    args = ap.parse_args()
    shapes = ([("lap3d-%d" % args.g3, (args.g3, args.g3, args.g3))] if args.g3 else []) + ([("lap2d-%d" % args.g2, (args.g2, args.g2, 1))] if args.g2 else [])
    for label, dims in shapes:
        for dt in args.dtypes.split(","):
            dtype = {"f32": np.float32, "f64": np.float64}[dt]
            natural = build(dims, dtype)
            for ordering in args.orderings.split(","):
                if ordering == "natural":
                    a = natural
                elif ordering == "color":
                    perm, stats = natural.color()
                    a = natural.permute_symmetric(perm)
                    a.sort_rows()  # (permute keeps each row's storage order: ilu0 wants ascending columns)
                    print("%s color %s: %d colours in %d rounds" % (label, np.dtype(dtype).name, stats["n_colors"], stats["n_rounds"]), flush=True)
                else:
                    a = natural.permute_symmetric(red_black_perm(dims))
                    a.sort_rows()
                run("%s %s" % (label, ordering), a, dtype, args)
                del a
            del natural
            check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
