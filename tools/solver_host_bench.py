#!/usr/bin/env python3
"""Ad-hoc: host wall time of one short, launch-bound solve per device-resident solver -- what the host side of a solver costs
(streams, workspaces, staging, capture, polls; csrc/solver_host.hpp).  7-point Laplacian g^3 f32, `--bodies` bodies at tol 0,
median (10th .. 90th percentile) of `--repeats` solves after `--warmup`.  To compare two trees, run it in each, alternating."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
try:  # (PyTorch's bundled HIP runtime initialises first, as in bench.py)
    import torch
    torch.cuda.init()
except Exception:
    pass
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=24)
    ap.add_argument("--bodies", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    g, it = args.grid, args.bodies
    n = g ** 3
    a = synth.crs_laplace3d(g, g, g, np.float32)
    f, _ = a.ilu0()
    fsai = a.fsai()[:2]   # (g, gt)
    bh, xh = np.ones(n, np.float32), np.zeros(n, np.float32)
    b, xd = sm.DenseVec.from_vec(bh), sm.DenseVec.zeros(n, np.float32)
    cases = [("cg_vec", lambda: sm.ConjugateGradient(0.0, it).solve(a, b, xd)),
             ("cg_host", lambda: sm.ConjugateGradient(0.0, it).solve(a, bh, xh)),
             ("jacobi_host", lambda: sm.JacobiConjugateGradient(0.0, it).solve(a, bh, xh)),
             ("sgs_vec", lambda: sm.SGSConjugateGradient(0.0, it).solve(a, b, xd)),
             ("ilu_vec", lambda: sm.ILUConjugateGradient(0.0, it).solve(a, b, xd, factor=f)),
             ("bicgstab_vec", lambda: sm.BiCGStab(0.0, it).solve(a, b, xd)),
             ("gmres_vec", lambda: sm.GMRES(0.0, it).solve(a, b, xd)),
             ("fsai_pcg_vec", lambda: sm.FSAIConjugateGradient(0.0, it).solve(a, b, xd, factor=fsai))]
    for kind, factor in (("sgs", None), ("ilu", f), ("fsai", fsai)):   # (the factors are built once, above)
        cases.append(("gmres_" + kind, lambda kind=kind, factor=factor: sm.GMRES(0.0, it, precond=kind).solve(a, b, xd, factor=factor)))
        cases.append(("bicgstab_" + kind, lambda kind=kind, factor=factor: sm.BiCGStab(0.0, it, precond=kind).solve(a, b, xd, factor=factor)))
    for name, fn in cases:
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts) * 1e6
        print("solver_host %d^3 f32, %d bodies: %-13s median %8.1f us  (p10 %8.1f .. p90 %8.1f)" % (
            g, it, name, np.median(ts), np.percentile(ts, 10), np.percentile(ts, 90)), flush=True)


if __name__ == "__main__":
    main()
