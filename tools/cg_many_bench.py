#!/usr/bin/env python3
"""Ad-hoc timing of the k-column conjugate gradient K5m on one GPU (development aid, not the contract bench):
``ConjugateGradient.solve_many`` on k right-hand sides against k calls of ``solve`` (``smh_cg_solve_vec`` through AUTO), f32 and
f64, k in {1, 2, 4, 8, 16}, tol 0 and a fixed count of 50 bodies -- so both sides do the same number of iterations whatever the
values do (the headline matrix is not SPD: its recurrence is run for its traffic, not for its solution).

Shapes: those of tools/mvp_many_bench.py -- the headline matrix (window pattern, 10 M rows x 32 entries); a 256^3 7-point
Laplacian with seeded non-constant coefficients; and the constant-coefficient Laplacian for information (there the single
product reads no values, and the byte model says the k-column solve does not win).

Timing: HIP events around one side's whole work -- one ``solve_many``, or the k ``solve``s one after the other; both are
synchronous calls on device-resident vectors, so the events bracket the set-up (r = b - A x, the workspaces), the 50 bodies and the
polls of each.  The two sides alternate in one process and every pairing runs `--repeats` times, so the spread is visible: the
ratio column gives min .. max over the repeats.  Before anything is printed column 0 of the k-column solve is compared bit for
bit with a k = 1 ``solve_many`` of the same right-hand side.  The byte model is printed beside each ratio."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import synth  # noqa: E402
from sparsemat_amd._lib import check, lib  # noqa: E402
from sparsemat_amd.multivec import leading_dim  # noqa: E402
import mvp_many_bench  # noqa: E402  (the shapes, their matrices and the products' byte model)

VECTOR_PASSES_MANY = 10        # per body beyond K1m's own X and Y: the dot 2, the update 3, the p sweep 5
VECTOR_PASSES_SINGLE = (8, 10)  # the single solver's tail: 8 with p.Ap out of the product's epilogue, 10 with a separate dot


class Events:
    def __init__(self):
        self.stream, self.a, self.b = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().smh_stream_create(C.byref(self.stream)))
        check(lib().smh_event_create(C.byref(self.a)))
        check(lib().smh_event_create(C.byref(self.b)))

    def ms(self, work):
        """`work` is synchronous: all of its device work lies between the two events."""
        check(lib().smh_device_synchronize())
        check(lib().smh_event_record(self.a, self.stream))
        work()
        check(lib().smh_event_record(self.b, self.stream))
        check(lib().smh_stream_synchronize(self.stream))
        ms = C.c_float()
        check(lib().smh_event_elapsed_ms(self.a, self.b, C.byref(ms)))
        return ms.value


def same(a, b):
    """bit equality, any NaN equal to any NaN"""
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def model_bytes(shape, vs, k):
    """Bytes per row and right-hand side of one body: (the k-column solve, the single solve's low and high end)."""
    many_prod, single_prod_k = mvp_many_bench.model_bytes(shape, vs, k)
    ld = leading_dim(k)
    many = (many_prod + VECTOR_PASSES_MANY * ld * vs) / k
    single = [single_prod_k / k + p * vs for p in VECTOR_PASSES_SINGLE]
    return many, single[0], single[1]


def run(shape, dtype, ks, args, ev):
    m = mvp_many_bench.build(shape, dtype)
    n, vs = m.n_rows(), np.dtype(dtype).itemsize
    m.prepare("auto")
    print("== %s %s: rows %d nnz %d auto=%s value dictionary %d; %d bodies at tol 0" % (
        shape["name"], np.dtype(dtype).name, n, m.n_non_zero_entries(), m.resolved_variant(), len(m.stream_value_dict()), args.bodies), flush=True)
    kmax = max(ks)
    bs = []
    for c in range(kmax):
        v = sm.DenseVec.zeros(n, dtype)
        synth.gen_x(synth.SEED_X + c, n, dtype, ptr=v.data_ptr())
        bs.append(v)
    cg = sm.ConjugateGradient(0.0, args.bodies)
    # the k = 1 solve of column 0: what column 0 of every k must be, bit for bit
    x1 = sm.MultiVec.zeros(n, 1, dtype)
    cg.solve_many(m, sm.MultiVec.from_vecs(bs[:1]), x1)
    x_ref = x1.column(0).to_numpy()
    del x1
    for k in ks:
        B = sm.MultiVec.from_vecs(bs[:k])
        t_many, t_single = [], []
        x_col0 = None
        for rep in range(args.repeats + 1):   # (the first pairing warms both sides up and is not counted)
            X = sm.MultiVec.zeros(n, k, dtype)
            tm = ev.ms(lambda: cg.solve_many(m, B, X))
            assert (cg.iterations == args.bodies).all()
            if x_col0 is None:
                x_col0 = X.column(0).to_numpy()
            del X
            xs = [sm.DenseVec.zeros(n, dtype) for _ in range(k)]

            def singles():
                for c in range(k):
                    cg.solve(m, bs[c], xs[c])

            ts = ev.ms(singles)
            assert cg.iterations == args.bodies
            del xs
            if rep:
                t_many.append(tm)
                t_single.append(ts)
        if not same(x_col0, x_ref):
            raise SystemExit("column 0 of the k = %d solve differs from the k = 1 solve" % k)
        mb, s_lo, s_hi = model_bytes(shape, vs, k)
        r = [a / b for a, b in zip(t_many, t_single)]
        med = lambda v: sorted(v)[len(v) // 2]
        print("  k=%-2d ld=%-2d solve_many %8.2f ms (%8.2f .. %8.2f) | k x solve %8.2f ms (%8.2f .. %8.2f) | many/singles %.3f (%.3f .. %.3f) spread %.1f%% | "
              "model %.0f / %.0f .. %.0f B per row and rhs = %.3f .. %.3f | solve_many %.0f GB/s by the model" % (
                  k, leading_dim(k), med(t_many), min(t_many), max(t_many), med(t_single), min(t_single), max(t_single), med(r), min(r), max(r),
                  100.0 * (max(r) - min(r)) / med(r), mb, s_lo, s_hi, mb / s_hi, mb / s_lo, mb * k * n * args.bodies / med(t_many) / 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000, help="rows of the headline matrix")
    ap.add_argument("--grid", type=int, default=256, help="edge of the Laplacian's grid")
    ap.add_argument("--shapes", default="headline,lap-varcoef,lap-const")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--bodies", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    shapes = {
        "headline": {"name": "headline", "rows": args.rows, "entries_per_row": 32, "single_offset_bytes": 4, "single_reads_no_values": False},
        "lap-varcoef": {"name": "lap-varcoef", "grid": args.grid, "entries_per_row": 7, "single_offset_bytes": 1, "single_reads_no_values": False},
        "lap-const": {"name": "lap-const", "grid": args.grid, "entries_per_row": 7, "single_offset_bytes": 1, "single_reads_no_values": True},
    }
    ev = Events()
    ks = [int(v) for v in args.ks.split(",")]
    print("SMH_MANY_KT8=%s" % os.environ.get("SMH_MANY_KT8", "0"))
    for name in args.shapes.split(","):
        for dt in args.dtypes.split(","):
            run(shapes[name], {"f32": np.float32, "f64": np.float64}[dt], ks, args, ev)
            check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
