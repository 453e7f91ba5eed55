#!/usr/bin/env python3
"""Ad-hoc timing of the non-symmetric FSAI (smh_crs_fsai_ns) and of GMRES and BiCGSTAB right-preconditioned by its pair
(smh_gmres_fsai_solve_vec, smh_bicgstab_fsai_solve_vec; extensions) on one GPU (development aid, not the contract bench).

Shape: tools/pgmres_bench.py's --shape convdiff, the 7-point Laplacian with upwind convection, in the NATURAL ordering -- the one in
which the triangular preconditioners are launch-bound and the product keeps its kernel.  The method is pgmres_bench.py's: all sides
alternate on one handle in one process; a warm-up round, then the median of --repeats rounds (HIP events around one synchronous
solve on device-resident vectors: set-up and polls included).

Tolerance block (tol = --rtol * |b|, from x0 = 0): GMRES(30) and BiCGSTAB unpreconditioned, with the FSAI pair of fsai_ns and with
ILU(0); then the same matrix with its rows scaled by 2^+-5 (tests/pgmres_model.scale_rows' rule): unpreconditioned, Jacobi, FSAI.
Per side: bodies, ms to tol, ms per body, and the true residual |b - A x| / |b| formed on the device in the working precision.

Separate timings: a fresh fsai_ns against a fresh fsai and a fresh ilu0 (wall clock around synchronous calls, the handle's forms
prepared before); the FSAI-GMRES body against the unpreconditioned one at fixed work (tol 0: the difference quotient of a solve of
one full cycle and one of three), next to the byte model's ratio -- a GMRES(m) body averaged over a cycle moves, beside its product,
(2 m + 11) + (m + 7) / m n-vectors; the pair adds two products whose rows hold 4 of the matrix's 7 entries and one
n-vector written and read between them, and the cycle end's pair 2 / m of that --; and the same body with the cycle end's gate
switched off (SMH_FSAI_END_GATE=0: every body then runs a second, dead pair through the handles' own products)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import synth  # noqa: E402
from sparsemat_amd._lib import check, lib  # noqa: E402
from cg_many_bench import Events  # noqa: E402
import mvp_many_bench  # noqa: E402  (the product's byte model)
import pgmres_bench  # noqa: E402  (the operator, wall)

RESTART = 30
med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
wall = pgmres_bench.wall


def to_tol(a, sides, b_host, tol, dtype, args, ev, label):
    """sides: (name, make solver, factor or None)"""
    n = a.n_rows()
    b = sm.DenseVec.from_vec(b_host)
    norm_b = float(np.linalg.norm(b_host.astype(np.float64)))
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
        print("    %-8s %-20s %5d bodies%s | %9.2f ms to tol (%.2f .. %.2f) | %7.3f ms per body | true residual %.2e |b|" % (
            label, name, bodies, " (breakdown %d)" % brk if brk else "", med(t), min(t), max(t), med(t) / max(bodies, 1), true), flush=True)


def fsai_body(a, pair, b_host, dtype, args, ev):
    n, vs = a.n_rows(), np.dtype(dtype).itemsize
    b = sm.DenseVec.from_vec(b_host)
    row = lambda entries: mvp_many_bench.model_bytes({"entries_per_row": entries, "single_offset_bytes": 1, "single_reads_no_values": False}, vs, 1)[1]
    product, factor_product = row(7), row(4)  # bytes per row of one product of the matrix / of a factor

    def per_body(precond, gate=None):
        t = []
        if gate is not None:
            os.environ["SMH_FSAI_END_GATE"] = gate
        try:
            for bodies in (RESTART, 3 * RESTART):
                x = sm.DenseVec.zeros(n, dtype)
                s = sm.GMRES(0.0, bodies, RESTART, precond=precond)
                t.append(ev.ms((lambda: s.solve(a, b, x, factor=pair)) if precond else (lambda: s.solve(a, b, x))))
                assert s.iterations == bodies, (s.iterations, bodies, s.breakdown)
        finally:
            os.environ.pop("SMH_FSAI_END_GATE", None)
        return (t[1] - t[0]) / (2 * RESTART)

    plain, fsai, open_gate = [], [], []
    for rep in range(args.repeats + 1):
        p, f, o = per_body(None), per_body("fsai"), per_body("fsai", "0")
        if rep:
            plain.append(p)
            fsai.append(f)
            open_gate.append(o)
    m = RESTART
    base = product + (2 * m + 11 + (m + 7) / m) * vs
    model = (base + (1 + 1.0 / m) * (2 * factor_product)) / base
    ratio = [f / p for f, p in zip(fsai, plain)]
    print("    body at fixed work: GMRES(30) %.3f ms (%.3f .. %.3f), + FSAI %.3f ms (%.3f .. %.3f): ratio %.4f (%.4f .. %.4f) against the "
          "byte model's %.4f" % (med(plain), min(plain), max(plain), med(fsai), min(fsai), max(fsai), med(ratio), min(ratio), max(ratio), model), flush=True)
    print("    ... with the cycle end's gate off (a dead pair through AUTO in every body): %.3f ms (%.3f .. %.3f), %.4f of the gated body" % (
        med(open_gate), min(open_gate), max(open_gate), med(open_gate) / med(fsai)), flush=True)


def factorizations(a, args):
    t = {"fsai_ns": [], "fsai": [], "ilu0": []}
    for rep in range(args.repeats + 1):
        for name in t:
            out, ms = wall(getattr(a, name))
            if rep:
                t[name].append(ms)
            del out
    print("    a fresh factorization: " + " | ".join("%s %.1f ms (%.1f .. %.1f)" % (k, med(v), min(v), max(v)) for k, v in t.items()), flush=True)


def run(dtype, args, ev):
    a = pgmres_bench.build(argparse.Namespace(shape="convdiff", grid=args.grid), dtype)
    n = a.n_rows()
    a.sort_rows()  # (ilu0 and fsai_ns need ascending rows; a no-op on this operator)
    a.prepare("auto")
    bd = sm.DenseVec.zeros(n, dtype)
    synth.gen_x(synth.SEED_X, n, dtype, ptr=bd.data_ptr())
    b = bd.to_numpy()
    tol = args.rtol[dtype] * float(np.linalg.norm(b.astype(np.float64)))
    print("convdiff %d^3 %s natural auto=%s: tol = %.1e |b| = %.3e" % (args.grid, np.dtype(dtype).name, a.resolved_variant(), args.rtol[dtype], tol), flush=True)
    factorizations(a, args)
    (gl, gu, singular), _ = wall(a.fsai_ns)
    (f, zp), _ = wall(a.ilu0)
    gl.prepare("auto")
    gu.prepare("auto")
    print("    fsai_ns: singular %s, G_L %d and G_U %d entries, auto=%s / %s | ilu0: zero pivot %s" % (
        singular, gl.n_non_zero_entries(), gu.n_non_zero_entries(), gl.resolved_variant(), gu.resolved_variant(), zp), flush=True)
    pair = (gl, gu)
    fsai_body(a, pair, b, dtype, args, ev)
    it = args.iter_max
    to_tol(a, [("GMRES(30)", lambda: sm.GMRES(tol, it, RESTART), None),
               ("GMRES(30) + FSAI", lambda: sm.GMRES(tol, it, RESTART, precond="fsai"), pair),
               ("GMRES(30) + ILU(0)", lambda: sm.GMRES(tol, it, RESTART, precond="ilu"), f),
               ("BiCGSTAB", lambda: sm.BiCGStab(tol, it), None),
               ("BiCGSTAB + FSAI", lambda: sm.BiCGStab(tol, it, precond="fsai"), pair),
               ("BiCGSTAB + ILU(0)", lambda: sm.BiCGStab(tol, it, precond="ilu"), f)], b, tol, dtype, args, ev, "as built")
    del f
    # the rows scaled by 2^k, k uniform in -5 .. 5 (exact); b is scaled with them, so the solution is the same
    off, col, val = a.raw_parts()
    k = np.random.default_rng(7).integers(-5, 6, n)
    scale = (2.0 ** k).astype(dtype)
    a.update_values(val * np.repeat(scale, np.diff(off.astype(np.int64))))
    del off, col, val
    bs = b * scale
    tol_s = args.rtol[dtype] * float(np.linalg.norm(bs.astype(np.float64)))
    (gl, gu, singular), _ = wall(a.fsai_ns)
    pair = (gl, gu)
    to_tol(a, [("GMRES(30)", lambda: sm.GMRES(tol_s, it, RESTART), None),
               ("GMRES(30) + Jacobi", lambda: sm.GMRES(tol_s, it, RESTART, precond="jacobi"), None),
               ("GMRES(30) + FSAI", lambda: sm.GMRES(tol_s, it, RESTART, precond="fsai"), pair),
               ("BiCGSTAB", lambda: sm.BiCGStab(tol_s, it), None),
               ("BiCGSTAB + Jacobi", lambda: sm.BiCGStab(tol_s, it, precond="jacobi"), None),
               ("BiCGSTAB + FSAI", lambda: sm.BiCGStab(tol_s, it, precond="fsai"), pair)], bs, tol_s, dtype, args, ev, "scaled")


def main():
    ap = argparse.ArgumentParser()
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
