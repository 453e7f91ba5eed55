#!/usr/bin/env python3
"""Ad-hoc timing of the device-resident BiCGSTAB (smh_bicgstab_solve_vec, an extension) on one GPU (development aid, not the
contract bench): ms per body next to the plain CG's ms per body on the same handle, in the same process, the two alternating.

Shapes: the 7-point Laplacian g^3 with seeded non-constant coefficients (tools/mvp_many_bench.py's "lap-varcoef"), and a
non-symmetric 7-point operator of the same size (its entries below the diagonal weigh 1.5 times as much: an upwinded
stencil; the diagonal is raised to keep the rows dominant).  f32 and f64.  tol 0 and fixed body counts, so both solvers do
the same work whatever the values do (CG's recurrence on the non-symmetric operator is run for its traffic, not for its
solution).

Timing: HIP events around one synchronous solve on device-resident vectors; a body's time is the difference quotient of two
body counts (set-up, workspaces and the last poll cancel).  Every pairing runs `--repeats` times after a warm-up pairing; the
ratio column gives the median and min .. max over the repeats.  The byte model beside it: one BiCGSTAB body = two products +
18 n values, one CG body = one product + 8 n values (p.Ap out of the product's epilogue)."""
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
import mvp_many_bench  # noqa: E402  (the Laplacian shapes and the product's byte model)

BICGSTAB_VALUES = 18  # per body beside the two products (BiCGSTAB)
CG_VALUES = 8         # per body beside the product


def build(name, grid, dtype):
    shape = {"name": "lap-varcoef", "grid": grid}
    m = mvp_many_bench.build(shape, dtype)
    if name == "lap-nonsym":
        off, col, val = m.raw_parts()
        rows = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off.astype(np.int64)))
        val = np.where(col < rows, val * 1.5, np.where(col == rows, val + 4.0, val)).astype(dtype)
        m.update_values(val)
    return m


def run(name, dtype, args, ev):
    m = build(name, args.grid, dtype)
    n, vs = m.n_rows(), np.dtype(dtype).itemsize
    m.prepare("auto")
    shape = {"entries_per_row": 7, "single_offset_bytes": 1, "single_reads_no_values": False}
    product = mvp_many_bench.model_bytes(shape, vs, 1)[1]  # bytes per row of one product
    model = (2 * product + BICGSTAB_VALUES * vs) / (product + CG_VALUES * vs)
    b = sm.DenseVec.zeros(n, dtype)
    synth.gen_x(synth.SEED_X, n, dtype, ptr=b.data_ptr())
    lo, hi = args.bodies, 3 * args.bodies

    def per_body(make):
        t = []
        for bodies in (lo, hi):
            x = sm.DenseVec.zeros(n, dtype)
            s = make(bodies)
            t.append(ev.ms(lambda: s.solve(m, b, x)))
            assert s.iterations == bodies, (s.iterations, bodies, getattr(s, "breakdown", None))
        return (t[1] - t[0]) / (hi - lo)

    t_bi, t_cg = [], []
    for rep in range(args.repeats + 1):  # (the first pairing warms both sides up and is not counted)
        bi = per_body(lambda k: sm.BiCGStab(0.0, k))
        cg = per_body(lambda k: sm.ConjugateGradient(0.0, k))
        if rep:
            t_bi.append(bi)
            t_cg.append(cg)
    r = [a / c for a, c in zip(t_bi, t_cg)]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    print("%s %d^3 %s auto=%s: BiCGSTAB %.3f ms per body (%.3f .. %.3f) | CG %.3f ms per body (%.3f .. %.3f) | ratio %.3f (%.3f .. %.3f) "
          "spread %.1f%% | model %.3f (%d against %d B per row) | BiCGSTAB %.0f GB/s by the model" % (
              name, args.grid, np.dtype(dtype).name, m.resolved_variant(), med(t_bi), min(t_bi), max(t_bi), med(t_cg), min(t_cg), max(t_cg),
              med(r), min(r), max(r), 100.0 * (max(r) - min(r)) / med(r), model, 2 * product + BICGSTAB_VALUES * vs, product + CG_VALUES * vs,
              (2 * product + BICGSTAB_VALUES * vs) * n / med(t_bi) / 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--shapes", default="lap-varcoef,lap-nonsym")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--bodies", type=int, default=20, help="the shorter solve; the longer one runs three times as many")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    ev = Events()
    for name in args.shapes.split(","):
        for dt in args.dtypes.split(","):
            run(name, {"f32": np.float32, "f64": np.float64}[dt], args, ev)
            check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
