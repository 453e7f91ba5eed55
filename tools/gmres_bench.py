#!/usr/bin/env python3
"""Ad-hoc timing of the device-resident restarted GMRES (smh_gmres_solve_vec, an extension) on one GPU (development aid, not the
contract bench): ms per body at restart 10, 30 and 50 next to BiCGSTAB's ms per body on the same handle, in the same process,
the sides alternating.

Shape: tools/bicgstab_bench.py's non-symmetric 7-point operator ("lap-nonsym"), f32 and f64.  tol 0 and fixed body counts, so every
solver does the same work whatever the values do.

Timing: HIP events around one synchronous solve on device-resident vectors; a GMRES(m) body's time is the difference quotient of a
solve of one full cycle (m bodies) and one of three (3 m): set-up, workspaces and the last poll cancel and what remains is a body
averaged over a cycle, the cycle end and the restart included.  BiCGSTAB: the difference quotient of `--bodies` and three times
as many.  Every round of all sides runs `--repeats` times after a warm-up round; medians and min .. max over the repeats.

The byte model beside it: a GMRES(m) body averaged over a cycle = one product + (2 m + 11) n values (dots and updates of both
Gram-Schmidt passes, the normalisation with its second copy for the product) + (m + 7) / m n values (the cycle end's sweep over the
basis, v_0); a BiCGSTAB body = two products + 18 n values.  "sweeps GB/s": the model's bytes beside the product over the body's
time less one product's time (the product timed alone through a CG body is not available here, so the product's share is taken
at the model's proportion of the BiCGSTAB body) -- an estimate, named as one."""
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
import bicgstab_bench  # noqa: E402  (the operator)
import mvp_many_bench  # noqa: E402  (the product's byte model)


def gmres_values(m):
    """n-vectors of values a GMRES(m) body moves beside its product, averaged over a full cycle"""
    return 2 * m + 11 + (m + 7) / m


def run(dtype, args, ev):
    m = bicgstab_bench.build("lap-nonsym", args.grid, dtype)
    n, vs = m.n_rows(), np.dtype(dtype).itemsize
    m.prepare("auto")
    shape = {"entries_per_row": 7, "single_offset_bytes": 1, "single_reads_no_values": False}
    product = mvp_many_bench.model_bytes(shape, vs, 1)[1]  # bytes per row of one product
    b = sm.DenseVec.zeros(n, dtype)
    synth.gen_x(synth.SEED_X, n, dtype, ptr=b.data_ptr())
    restarts = [int(r) for r in args.restarts.split(",")]

    def per_body(make, lo, hi):
        t = []
        for bodies in (lo, hi):
            x = sm.DenseVec.zeros(n, dtype)
            s = make(bodies)
            t.append(ev.ms(lambda: s.solve(m, b, x)))
            assert s.iterations == bodies, (s.iterations, bodies, getattr(s, "breakdown", None))
        return (t[1] - t[0]) / (hi - lo)

    t_bi, t_gm = [], {r: [] for r in restarts}
    for rep in range(args.repeats + 1):  # (the first round warms every side up and is not counted)
        bi = per_body(lambda k: sm.BiCGStab(0.0, k), args.bodies, 3 * args.bodies)
        gm = {r: per_body(lambda k, r=r: sm.GMRES(0.0, k, restart=r), r, 3 * r) for r in restarts}
        if rep:
            t_bi.append(bi)
            for r in restarts:
                t_gm[r].append(gm[r])
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    bi_bytes = 2 * product + bicgstab_bench.BICGSTAB_VALUES * vs
    print("lap-nonsym %d^3 %s auto=%s: BiCGSTAB %.3f ms per body (%.3f .. %.3f), %d B per row, %.0f GB/s by the model" % (
        args.grid, np.dtype(dtype).name, m.resolved_variant(), med(t_bi), min(t_bi), max(t_bi), bi_bytes, bi_bytes * n / med(t_bi) / 1e6), flush=True)
    for r in restarts:
        t = t_gm[r]
        ratio = [g / c for g, c in zip(t, t_bi)]
        gm_bytes = product + gmres_values(r) * vs
        product_ms = med(t_bi) * product / bi_bytes  # (the product's share of a BiCGSTAB body by the model: an estimate)
        sweeps = gmres_values(r) * vs * n / max(med(t) - product_ms, 1e-9) / 1e6
        print("    GMRES(%d) %.3f ms per body (%.3f .. %.3f) | against BiCGSTAB %.3f (%.3f .. %.3f) spread %.1f%% | model %.3f (%.0f against %d B "
              "per row) | %.0f GB/s by the model | sweeps alone about %.0f GB/s" % (
                  r, med(t), min(t), max(t), med(ratio), min(ratio), max(ratio), 100.0 * (max(ratio) - min(ratio)) / med(ratio),
                  gm_bytes / bi_bytes, gm_bytes, bi_bytes, gm_bytes * n / med(t) / 1e6, sweeps), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--restarts", default="10,30,50")
    ap.add_argument("--bodies", type=int, default=20, help="BiCGSTAB's shorter solve; the longer one runs three times as many")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    ev = Events()
    for dt in args.dtypes.split(","):
        run({"f32": np.float32, "f64": np.float64}[dt], args, ev)
        check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
