#!/usr/bin/env python3
"""Ad-hoc timing of the factorized sparse approximate inverse and the CG it preconditions (smh_crs_fsai, smh_crs_fsai_apply_vec,
smh_pcg_fsai_solve: extensions) on one GPU (development aid, not the contract bench), with the method of tools/ilu_bench.py: the
sides of every comparison alternate in one process; medians with min .. max over `--repeats` rounds after a warm-up round.

Matrices, f32 and f64, natural ordering: tools/sgs_bench.py's 7-point operator on g3^3 and 5-point operator on g2^2 (hashed edge
weights: non-constant coefficients).

Per matrix: the build -- a fresh fsai (count, scan, emit, the rows' sweep, the transposition and both handles' create-time
inspection: wall) in alternation with a fresh ilu0 and one AUTO product of A, against its byte model (A's offsets, columns and
values read once, G's and G^T's offsets, columns and values written once, G read once by the transposition); the application -- a
G + G^T product pair (fsai_apply) in alternation with one AUTO product of A and an SGS LOWER + UPPER solve pair; then wall time and
bodies to tol for CG, Jacobi-PCG, SGS-PCG, ILU-PCG and FSAI-PCG (the factors made before and passed in) from x0 = 0, host vectors
for all five, the five solvers alternating.

`--parts` instead: what a fresh fsai is made of -- the whole in alternation with a transposition of G (the bucketed passes and the
new handle's create-time inspection) and a clone of G (a copy and that inspection alone); what remains of the whole is the pattern
check, count, scan, emit and the rows' sweep."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sgs_bench import build, med, spread, wall_ms  # noqa: E402
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import _lib  # noqa: E402
from sparsemat_amd._lib import check, lib  # noqa: E402


def run(label, a, dtype, args):
    n, nnz = a.n_rows(), a.n_non_zero_entries()
    vs = np.dtype(dtype).itemsize
    name = "%s %s" % (label, np.dtype(dtype).name)
    a.prepare("auto")
    made = {}
    t_first = wall_ms(lambda: made.update(f=a.fsai()))
    g, gt, not_spd = made["f"]
    g.prepare("auto")
    gt.prepare("auto")
    nnz_g = g.n_non_zero_entries()
    print("%s: n %d nnz %d auto=%s | G nnz %d auto=%s | G^T auto=%s | not_spd %s | first fsai %.1f ms" % (
        name, n, nnz, a.resolved_variant(), nnz_g, g.resolved_variant(), gt.resolved_variant(), not_spd, t_first), flush=True)
    if args.parts:
        t_all, t_tr, t_cl = [], [], []
        for rep in range(args.repeats + 1):
            p, q, r = wall_ms(lambda: a.fsai()), wall_ms(lambda: g.transpose()), wall_ms(lambda: g.clone())
            if rep:
                t_all.append(p), t_tr.append(q), t_cl.append(r)
        print("%s: fresh fsai %s ms | transpose(G) %s ms (route %s) | clone(G) %s ms | fsai - transpose(G) - clone(G) %.3f ms" % (
            name, spread(t_all), spread(t_tr), sm.SparseMatCRS.last_transpose_route(), spread(t_cl), med(t_all) - med(t_tr) - med(t_cl)), flush=True)
        return
    rng = np.random.default_rng(5)
    b_host = rng.uniform(-1.0, 1.0, n).astype(dtype)
    b, w, y = sm.DenseVec.from_vec(b_host), sm.DenseVec.zeros(n, dtype), sm.DenseVec.zeros(n, dtype)
    L = lib()

    def product():
        a.mvp_dev(b.data_ptr(), n, y.data_ptr(), "auto")

    # the build
    model_bytes = (n + 1) * 4 + nnz * (4 + vs) + 3 * ((n + 1) * 4 + nnz_g * (4 + vs))
    t_fsai, t_ilu, t_prod = [], [], []
    for rep in range(args.repeats + 1):
        p, q, r = wall_ms(lambda: a.fsai()), wall_ms(lambda: a.ilu0()), wall_ms(product)
        if rep:
            t_fsai.append(p), t_ilu.append(q), t_prod.append(r)
    print("%s: fresh fsai %s ms | fresh ilu0 %s ms | one AUTO product of A %s ms | fsai / product %.1f | byte model %.1f MB = %.3f ms at 4 TB/s" % (
        name, spread(t_fsai), spread(t_ilu), spread(t_prod), med(t_fsai) / med(t_prod), model_bytes / 1e6, model_bytes / 4e12 * 1e3), flush=True)

    # the application
    def fsai_pair():
        check(L.smh_crs_fsai_apply_vec(g._h, gt._h, b._h, w._h))

    def sgs_pair():
        check(L.smh_crs_trisolve_vec(a._h, _lib.SMH_TRI_LOWER, _lib.SMH_DIAG_NON_UNIT, b._h, w._h))
        check(L.smh_crs_trisolve_vec(a._h, _lib.SMH_TRI_UPPER, _lib.SMH_DIAG_NON_UNIT, w._h, w._h))

    sgs_pair()  # (the schedules' build is not the pair's time)
    t_pair, t_prod, t_sgs = [], [], []
    for rep in range(args.repeats + 1):
        p, q, r = wall_ms(fsai_pair), wall_ms(product), wall_ms(sgs_pair)
        if rep:
            t_pair.append(p), t_prod.append(q), t_sgs.append(r)
    print("%s: G + G^T product pair %s ms | one AUTO product of A %s ms | pair / product %.2f | SGS LOWER + UPPER pair %s ms | SGS pair / FSAI pair %.1f" % (
        name, spread(t_pair), spread(t_prod), med(t_pair) / med(t_prod), spread(t_sgs), med(t_sgs) / med(t_pair)), flush=True)

    # the solvers
    f, _ = a.ilu0()
    norm_b = float(np.sqrt(np.sum(b_host.astype(np.float64) ** 2)))
    tol = (args.tol32 if dtype == np.float32 else args.tol64) * norm_b
    solvers = (("CG", sm.ConjugateGradient, {}), ("Jacobi-PCG", sm.JacobiConjugateGradient, {}), ("SGS-PCG", sm.SGSConjugateGradient, {}),
               ("ILU-PCG", sm.ILUConjugateGradient, {"factor": f}), ("FSAI-PCG", sm.FSAIConjugateGradient, {"factor": (g, gt)}))
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--iter-max", type=int, default=5000)
    ap.add_argument("--tol32", type=float, default=1e-4, help="relative to |b|")
    ap.add_argument("--tol64", type=float, default=1e-8)
    ap.add_argument("--parts", action="store_true", help="only: a fresh fsai against a transposition and a clone of G")
    args = ap.parse_args()
    shapes = ([("lap3d-%d" % args.g3, (args.g3, args.g3, args.g3))] if args.g3 else []) + ([("lap2d-%d" % args.g2, (args.g2, args.g2, 1))] if args.g2 else [])
    for label, dims in shapes:
        for dt in args.dtypes.split(","):
            dtype = {"f32": np.float32, "f64": np.float64}[dt]
            a = build(dims, dtype)
            run("%s natural" % label, a, dtype, args)
            del a
            check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
