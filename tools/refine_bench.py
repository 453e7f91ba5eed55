#!/usr/bin/env python3
"""Ad-hoc timing of mixed-precision iterative refinement (smh_refine_solve_vec; an extension) against the f64 solvers on one GPU
(development aid, not the contract bench).

--case cg        the 7-point operator with non-constant coefficients on grid^3 (tools/sgs_bench.build, the operator of fsai_bench.py):
                 the f64 ConjugateGradient against IterativeRefinement(inner="cg")
--case convdiff  the convection-diffusion operator of tools/pbicgstab_bench.py on grid^3: f64 BiCGSTAB against refinement with f32
                 BiCGSTAB, and f64 FSAI-GMRES(30) against refinement with f32 FSAI-GMRES(30)

Both sides of a pair run to the same absolute tolerance, --rtol |b| (default 1e-8), from x0 = 0 on device-resident vectors, in one
process, alternating: a warm-up round (forms, plans, pooled memory), then the median of --repeats rounds with the spread (wall clock
around one synchronous solve, the device synchronised at both ends: set-up and polls included).  The f32 matrix and the factors are
made before the clock starts; the cast is timed on its own.  Per side: bodies (refinement: the inner solves' total), outer steps, ms
to tolerance, and the true |b - A x| / |b| with the product and the norm in f64.  Extra memory of refinement: the f32 copy (values,
columns, offsets; its derived forms come on top as for any handle) and five work vectors (three f64, two f32) beside the inner
solver's own f32 workspaces."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import synth  # noqa: E402
from sparsemat_amd._lib import check, lib  # noqa: E402
from sgs_bench import build as build_laplace, med, wall_ms  # noqa: E402
import pbicgstab_bench  # noqa: E402

F32, F64 = np.float32, np.float64


def compare(a, b_host, tol, sides, repeats):
    """sides: (name, make solver, solve(solver, b, x)); alternating, the first round not counted"""
    n = a.n_rows()
    b = sm.DenseVec.from_vec(b_host)
    norm_b = float(np.linalg.norm(b_host))
    ms, info = {name: [] for name, _, _ in sides}, {}
    for rep in range(repeats + 1):
        for name, make, solve in sides:
            x = sm.DenseVec.zeros(n, F64)
            s = make()
            t = wall_ms(lambda: solve(s, b, x))
            if rep:
                ms[name].append(t)
            true = float(np.linalg.norm(b_host - a.mvp(x.to_numpy()))) / norm_b
            info[name] = (s.iterations, getattr(s, "outer_iterations", None), getattr(s, "code", getattr(s, "breakdown", 0)), true)
    for name, _, _ in sides:
        bodies, outer, code, true = info[name]
        t = ms[name]
        print("    %-34s %6d bodies%s (code %s) | %9.2f ms to tol (%.2f .. %.2f) | true residual %.2e |b| (tol %.1e |b|)" % (
            name, bodies, " in %d outer steps" % outer if outer is not None else "", code, med(t), min(t), max(t), true, tol / norm_b), flush=True)
    first, second = sides[0][0], sides[1][0]
    print("    %s / %s: %.3f of the time, %.3f of the bodies" % (second, first, med(ms[second]) / med(ms[first]), info[second][0] / max(info[first][0], 1)), flush=True)


def prepare(a, args):
    """b, tol, the f32 copy (timed) and the extra memory"""
    n, nnz = a.n_rows(), a.n_non_zero_entries()
    a.prepare("auto")
    bd = sm.DenseVec.zeros(n, F64)
    synth.gen_x(synth.SEED_X, n, F64, ptr=bd.data_ptr())
    b = bd.to_numpy()
    tol = args.rtol * float(np.linalg.norm(b))
    casts = []
    for _ in range(args.repeats + 1):
        box = []
        casts.append(wall_ms(lambda: box.append(a.astype(F32))))
        a_lo = box[0]
    a_lo.prepare("auto")
    copy = nnz * 8 + (n + 1) * 4
    print("    n = %d, nnz = %d, f64 auto=%s, f32 auto=%s | cast %.2f ms (%.2f .. %.2f after the first, %.2f) | extra memory: f32 copy %.1f MiB + "
          "work vectors %.1f MiB (the f64 handle's arrays: %.1f MiB)" % (n, nnz, a.resolved_variant(), a_lo.resolved_variant(), med(casts[1:]), min(casts[1:]),
                                                                        max(casts[1:]), casts[0], copy / 2 ** 20, n * 32 / 2 ** 20, (nnz * 12 + (n + 1) * 4) / 2 ** 20),
          flush=True)
    return b, tol, a_lo


def run_cg(args):
    g = args.grid
    a = build_laplace((g, g, g), F64)
    print("7-point operator with non-constant coefficients, %d^3, to %.0e |b|" % (g, args.rtol), flush=True)
    b, tol, a_lo = prepare(a, args)
    it = args.iter_max
    compare(a, b, tol, [
        ("f64 CG", lambda: sm.ConjugateGradient(tol, it), lambda s, bb, x: s.solve(a, bb, x)),
        ("refinement, f32 CG inside", lambda: sm.IterativeRefinement(tol, inner="cg", inner_tol=args.inner_tol, inner_iter_max=it),
         lambda s, bb, x: s.solve(a, bb, x, mat_lo=a_lo)),
    ], args.repeats)


def run_convdiff(args):
    g = args.grid
    a, _ = pbicgstab_bench.build(argparse.Namespace(grid=g, convection=args.convection), F64, False)
    a.sort_rows()
    print("convection-diffusion (c = %g), %d^3, to %.0e |b|" % (args.convection, g, args.rtol), flush=True)
    b, tol, a_lo = prepare(a, args)
    it = args.iter_max
    compare(a, b, tol, [
        ("f64 BiCGSTAB", lambda: sm.BiCGStab(tol, it), lambda s, bb, x: s.solve(a, bb, x)),
        ("refinement, f32 BiCGSTAB inside", lambda: sm.IterativeRefinement(tol, inner="bicgstab", inner_tol=args.inner_tol, inner_iter_max=it),
         lambda s, bb, x: s.solve(a, bb, x, mat_lo=a_lo)),
    ], args.repeats)
    pair = a.fsai_ns()[:2]
    pair_lo = a_lo.fsai_ns()[:2]
    for f in pair + pair_lo:
        f.prepare("auto")
    compare(a, b, tol, [
        ("f64 FSAI-GMRES(30)", lambda: sm.GMRES(tol, it, 30, precond="fsai"), lambda s, bb, x: s.solve(a, bb, x, factor=pair)),
        ("refinement, f32 FSAI-GMRES(30) inside", lambda: sm.IterativeRefinement(tol, inner="gmres", precond="fsai", inner_tol=args.inner_tol, inner_iter_max=it,
                                                                              restart=30),
         lambda s, bb, x: s.solve(a, bb, x, mat_lo=a_lo, factor=pair_lo)),
    ], args.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("cg", "convdiff"), default="cg")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--inner-tol", type=float, default=1e-4)
    ap.add_argument("--convection", type=float, default=1.0)
    ap.add_argument("--iter-max", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    (run_cg if args.case == "cg" else run_convdiff)(args)
    check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
