#!/usr/bin/env python3
"""Ad-hoc timing of the level-scheduled triangular solves and the SGS-preconditioned CG (smh_crs_trisolve*, smh_pcg_sgs_solve,
extensions) on one GPU (development aid, not the contract bench).  The sides of every comparison alternate in one process;
medians with min .. max over `--repeats` pairings after a warm-up pairing.

Matrices, f32 and f64: the 7-point operator on g3^3 and the 5-point operator on g2^2 with non-constant coefficients (every edge
a weight 10^u, u in (-0.5, 0.5) by a hash of its end points, stored as -w and added to both end points' diagonals; diagonal
shift 0.05: SPD, the shape of tests/sgs_model.py's lap2d), each in the natural ordering and renumbered red-black (a stable sort
by (i + j + k) mod 2 through permute_symmetric).

Per matrix: the schedule's build time (wall, both triangles, first use) with its level and launch counts; a LOWER + UPPER solve
pair against one AUTO product of the same handle; an SGS-PCG body against a Jacobi-PCG body (difference quotient of two body
counts at tol 0 -- 10 and 30 SGS bodies, 200 and 600 Jacobi bodies --: set-up and copies cancel); wall time and bodies to tol for CG, Jacobi-PCG and SGS-PCG from x0 = 0 (host
vectors for all three: the copies are the same)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import synth  # noqa: E402
from sparsemat_amd._lib import check, lib  # noqa: E402


def wall_ms(work):
    check(lib().smh_device_synchronize())
    t = time.perf_counter()
    work()
    check(lib().smh_device_synchronize())
    return (time.perf_counter() - t) * 1e3


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (med(v), min(v), max(v))


def build(dims, dtype):
    """The grid operator with hashed edge weights; values computed on the host from the device-built pattern."""
    nx, ny, nz = dims
    m = synth.crs_laplace3d(nx, ny, nz, dtype)
    off, col, _ = m.raw_parts()
    n = len(off) - 1
    rows = np.repeat(np.arange(n, dtype=np.uint32), np.diff(off.astype(np.int64)))
    lo, hi = np.minimum(rows, col).astype(np.uint64), np.maximum(rows, col).astype(np.uint64)
    h = (lo * np.uint64(2654435761) + hi * np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    w = 10.0 ** (h.astype(np.float64) / 2.0 ** 32 - 0.5)
    diag = rows == col
    w[diag] = 0.0
    d = 0.05 + np.bincount(rows, weights=w, minlength=n)
    val = np.where(diag, d[rows], -w).astype(dtype)
    del lo, hi, h, w, d
    a = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    return a


def red_black_perm(dims):
    nx, ny, nz = dims
    idx = np.arange(nx * ny * nz, dtype=np.int64)
    k = idx % nz
    j = (idx // nz) % ny
    i = idx // (nz * ny)
    return np.argsort((i + j + k) % 2, kind="stable").astype(np.uint32)


def run(label, a, dtype, args):
    n = a.n_rows()
    name = "%s %s" % (label, np.dtype(dtype).name)
    t_build = wall_ms(lambda: (a.trisolve_levels("lower"), a.trisolve_levels("upper")))
    lo, up = a.trisolve_levels("lower"), a.trisolve_levels("upper")
    a.prepare("auto")
    print("%s: n %d nnz %d auto=%s | schedule build (both triangles) %.1f ms | levels %d / %d | launches per solve %d / %d (R = %d)" % (
        name, n, a.n_non_zero_entries(), a.resolved_variant(), t_build, lo["n_levels"], up["n_levels"], lo["n_launches"], up["n_launches"],
        lo["small_level_rows"]), flush=True)
    rng = np.random.default_rng(5)
    b_host = rng.uniform(-1.0, 1.0, n).astype(dtype)
    b = sm.DenseVec.from_vec(b_host)
    w, y = sm.DenseVec.zeros(n, dtype), sm.DenseVec.zeros(n, dtype)
    L = lib()
    from sparsemat_amd import _lib

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
    print("%s: LOWER + UPPER solve pair %s ms | one AUTO product %s ms | ratio %.1f" % (name, spread(t_pair), spread(t_prod), med(t_pair) / med(t_prod)),
          flush=True)

    def per_body(cls, scale=1):
        t = []
        for bodies in (scale * args.bodies, 3 * scale * args.bodies):
            x = np.zeros(n, dtype)
            s = cls(0.0, bodies)
            t.append(wall_ms(lambda: s.solve(a, b_host, x)))
            assert s.iterations == bodies, (s.iterations, bodies)
        return (t[1] - t[0]) / (2 * scale * args.bodies)

    t_sgs, t_jac = [], []
    for rep in range(args.repeats + 1):
        p, q = per_body(sm.SGSConjugateGradient), per_body(sm.JacobiConjugateGradient, 20)  # (a Jacobi body is short: more of them)
        if rep:
            t_sgs.append(p)
            t_jac.append(q)
    print("%s: SGS-PCG body %s ms | Jacobi-PCG body %s ms | ratio %.2f" % (name, spread(t_sgs), spread(t_jac), med(t_sgs) / med(t_jac)), flush=True)

    tol = (args.tol32 if dtype == np.float32 else args.tol64) * float(np.sqrt(np.sum(b_host.astype(np.float64) ** 2)))
    out = []
    for what, cls in (("CG", sm.ConjugateGradient), ("Jacobi-PCG", sm.JacobiConjugateGradient), ("SGS-PCG", sm.SGSConjugateGradient)):
        ts, its, rr = [], None, None
        for rep in range(args.solve_repeats):
            x = np.zeros(n, dtype)
            s = cls(tol, args.iter_max)
            ts.append(wall_ms(lambda: s.solve(a, b_host, x)))
            its, rr = s.iterations, s.r_norm_squared
        out.append("%s %d bodies %s ms%s" % (what, its, spread(ts), "" if np.sqrt(rr) < tol else " (NOT converged: |r| %.3g)" % np.sqrt(rr)))
    print("%s: to |r| < %.3g (%.0e |b|): %s" % (name, tol, tol / float(np.sqrt(np.sum(b_host.astype(np.float64) ** 2))), " | ".join(out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g3", type=int, default=256, help="the 7-point operator's grid (g3^3)")
    ap.add_argument("--g2", type=int, default=1024, help="the 5-point operator's grid (g2^2)")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--orderings", default="natural,red-black")
    ap.add_argument("--bodies", type=int, default=10, help="the shorter fixed-count solve; the longer one runs three times as many")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--solve-repeats", type=int, default=2)
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
                a = natural if ordering == "natural" else natural.permute_symmetric(red_black_perm(dims))
                run("%s %s" % (label, ordering), a, dtype, args)
                del a
            del natural
            check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
