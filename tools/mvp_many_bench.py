#!/usr/bin/env python3
"""Ad-hoc timing of the multi-vector product K1m on one GPU (development aid, not the contract bench): ``mvp_many`` on k
right-hand sides against k single products through AUTO and against k through STREAM, f32 and f64, k in {1, 2, 3, 4, 8, 16}.

Shapes: the headline matrix (window pattern, 10 M rows x 32 entries); a 256^3 7-point Laplacian whose values were replaced by
seeded non-constant coefficients (more than 32 distinct values: the value dictionary of K1s XD-V does not apply, the single
product reads the values); and the constant-coefficient Laplacian for information (there the single product reads no values).

Timing: HIP events around `--launches` launches after a warm-up; the three sides alternate in one process and every pairing is
repeated `--repeats` times, so the spread is visible: the ratio column gives min .. max over the repeats.  Before anything is
reported the results are compared on sampled rows: K1m against STREAM bit for bit, against AUTO within rounding.  The byte model
(what each side must move per row) is printed beside each measured ratio."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import _lib, synth  # noqa: E402
from sparsemat_amd._lib import check, lib  # noqa: E402
from sparsemat_amd.multivec import leading_dim  # noqa: E402


class Timer:
    def __init__(self):
        self.stream, self.a, self.b = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().smh_stream_create(C.byref(self.stream)))
        check(lib().smh_event_create(C.byref(self.a)))
        check(lib().smh_event_create(C.byref(self.b)))

    def ms_per_launch(self, launch, launches, warm):
        for _ in range(warm):
            launch(self.stream.value)
        check(lib().smh_stream_synchronize(self.stream))
        check(lib().smh_event_record(self.a, self.stream))
        for _ in range(launches):
            launch(self.stream.value)
        check(lib().smh_event_record(self.b, self.stream))
        check(lib().smh_stream_synchronize(self.stream))
        ms = C.c_float()
        check(lib().smh_event_elapsed_ms(self.a, self.b, C.byref(ms)))
        return ms.value / launches


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def model_bytes(shape, vs, k):
    """(bytes per row of one mvp_many, bytes per row of k single products): the entries' columns and values, the row offset,
    x and y.  Single products stream 16-bit columns on all three shapes (K1r's col16 / K1s's codes), a byte per row for its
    length on the stencils, and no values at all on the constant-coefficient stencil (value dictionary); K1m streams the u32
    columns, the values and the u32 offset once per sweep of 4 columns, and ld entries of X and of Y."""
    e = shape["entries_per_row"]
    ld = leading_dim(k)
    many = (ld // 4) * (e * (4 + vs) + 4) + 2 * ld * vs
    single = e * (2 + (0 if shape["single_reads_no_values"] else vs)) + shape["single_offset_bytes"] + 2 * vs
    return many, k * single


def build(shape, dtype):
    if shape["name"] == "headline":
        return synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, shape["rows"], 32, dtype)
    g = shape["grid"]
    m = synth.crs_laplace3d(g, g, g, dtype)
    if shape["name"] == "lap-varcoef":
        rng = np.random.default_rng(0x5EED)
        m.update_values(rng.uniform(0.5, 1.5, m.n_non_zero_entries()).astype(dtype))
    return m


def run(shape, dtype, ks, args, timer):
    m = build(shape, dtype)
    n, vs = m.n_rows(), np.dtype(dtype).itemsize
    m.prepare("auto")
    m.prepare("stream")
    print("== %s %s: rows %d nnz %d auto=%s value dictionary %d" % (shape["name"], np.dtype(dtype).name, n, m.n_non_zero_entries(),
                                                                     m.resolved_variant(), len(m.stream_value_dict())), flush=True)
    kmax = max(ks)
    xs = []
    for c in range(kmax):
        v = sm.DenseVec.zeros(n, dtype)
        synth.gen_x(synth.SEED_X + c, n, dtype, ptr=v.data_ptr())
        xs.append(v)
    ys_auto = [sm.DenseVec.zeros(n, dtype) for _ in range(kmax)]
    ys_stream = [sm.DenseVec.zeros(n, dtype) for _ in range(kmax)]
    sample = np.arange(0, n, max(1, n // args.sample_rows))
    for k in ks:
        X = sm.MultiVec.from_vecs(xs[:k])
        Y = sm.MultiVec.zeros(n, k, dtype)
        ld = X.ld()

        def many(st):
            m.mvp_many_dev(X.data_ptr(), n, Y.data_ptr(), k, ld, stream=st)

        def singles(variant, ys):
            def f(st):
                for c in range(k):
                    m.mvp_dev(xs[c].data_ptr(), n, ys[c].data_ptr(), variant, stream=st)
            return f

        t = {"many": [], "auto": [], "stream": []}
        for _ in range(args.repeats):  # the sides alternate; every pairing is repeated
            t["many"].append(timer.ms_per_launch(many, args.launches, args.warmup))
            t["auto"].append(timer.ms_per_launch(singles("auto", ys_auto), args.launches, args.warmup))
            t["stream"].append(timer.ms_per_launch(singles("stream", ys_stream), args.launches, args.warmup))
        # the results, on sampled rows, before anything is reported
        for c in sorted({0, k // 2, k - 1}):
            ym = Y.column(c).to_numpy()[sample]
            ysr = ys_stream[c].to_numpy()[sample]
            ya = ys_auto[c].to_numpy()[sample]
            if not np.array_equal(bits(ym), bits(ysr)):
                raise SystemExit("K1m and STREAM differ in column %d (%d of %d sampled rows)" % (c, (bits(ym) != bits(ysr)).sum(), len(sample)))
            tol = (1e-5 if dtype == np.float32 else 1e-12) * shape["entries_per_row"] * 8.0
            if not (np.abs(ym.astype(np.float64) - ya.astype(np.float64)) <= tol * np.maximum(1.0, np.abs(ya))).all():
                raise SystemExit("K1m and AUTO differ beyond rounding in column %d" % c)
        mb, sb = model_bytes(shape, vs, k)
        ra = [a / b for a, b in zip(t["many"], t["auto"])]
        rs = [a / b for a, b in zip(t["many"], t["stream"])]
        med = lambda v: sorted(v)[len(v) // 2]
        print("  k=%-2d ld=%-2d many %7.3f ms (%7.3f .. %7.3f) | k x AUTO %7.3f ms (%7.3f .. %7.3f) | k x STREAM %7.3f ms | many/AUTO %.3f (%.3f .. %.3f) "
              "spread %.1f%% | many/STREAM %.3f | model %d / %d B per row = %.3f | K1m %.0f GB/s" % (
                  k, ld, med(t["many"]), min(t["many"]), max(t["many"]), med(t["auto"]), min(t["auto"]), max(t["auto"]), med(t["stream"]),
                  med(ra), min(ra), max(ra), 100.0 * (max(ra) - min(ra)) / med(ra), med(rs), mb, sb, mb / sb, mb * n / med(t["many"]) / 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000, help="rows of the headline matrix")
    ap.add_argument("--grid", type=int, default=256, help="edge of the Laplacian's grid")
    ap.add_argument("--shapes", default="headline,lap-varcoef,lap-const")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--ks", default="1,2,3,4,8,16")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample-rows", type=int, default=20_000)
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("at least 20 launches between the events")
    shapes = {
        "headline": {"name": "headline", "rows": args.rows, "entries_per_row": 32, "single_offset_bytes": 4, "single_reads_no_values": False},
        "lap-varcoef": {"name": "lap-varcoef", "grid": args.grid, "entries_per_row": 7, "single_offset_bytes": 1, "single_reads_no_values": False},
        "lap-const": {"name": "lap-const", "grid": args.grid, "entries_per_row": 7, "single_offset_bytes": 1, "single_reads_no_values": True},
    }
    timer = Timer()
    ks = [int(v) for v in args.ks.split(",")]
    print("SMH_MANY_KT8=%s" % os.environ.get("SMH_MANY_KT8", "0"))
    for name in args.shapes.split(","):
        for dt in args.dtypes.split(","):
            run(shapes[name], {"f32": np.float32, "f64": np.float64}[dt], ks, args, timer)
            check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
