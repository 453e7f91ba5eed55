#!/usr/bin/env python3
"""Ad-hoc measurement of the reordering operations on one GPU (development aid, not the contract bench; nothing here is a pass /
fail bar): what does it cost to bring a randomly renumbered matrix back into an order with column locality, and what does the
product gain?

Inputs, both f32: the headline matrix (window pattern, 10 M rows x 32 entries) and a 256^3 7-point operator with seeded
non-constant coefficients, each renumbered by a random permutation through ``permute_symmetric`` itself.

Per input: the wall time of ``rcm`` and of ``permute_symmetric`` (both have finished when they return), ``prepare`` of the
reordered matrix, the AUTO product time of the renumbered, the reordered and the original matrix -- the three alternate in one
process, HIP events around `--launches` launches after a warm-up, median of `--repeats` with the spread -- which variant each
resolves to, and the number of products after which reordering has paid for itself,
(rcm + permute + prepare) / (t_renumbered - t_reordered).

The emit pass of ``permute`` against its byte model (DESIGN.md "Reordering"): ``permute()`` with both permutations None runs the
row lengths, the scan and the emit pass and then the same create-time inspection as ``clone()``, whose three device copies are the
copy ceiling; both wall times and the bytes they move are printed.  The emit pass alone is not timed.

When the reordered matrix does not resolve as the original does, the histogram of the 64-row tile spans of both is printed."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsemat_amd as sm  # noqa: E402
from sparsemat_amd import synth  # noqa: E402
from sparsemat_amd._lib import check, lib  # noqa: E402


class Tee:
    def __init__(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.f = open(path, "w")

    def __call__(self, text=""):
        print(text, flush=True)
        self.f.write(text + "\n")
        self.f.flush()


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


def wall_ms(f):
    check(lib().smh_device_synchronize())
    t0 = time.perf_counter()
    r = f()
    check(lib().smh_device_synchronize())
    return r, (time.perf_counter() - t0) * 1e3


def build(name, dtype):
    if name == "headline":
        return synth.crs_fixed(synth.SEED_MATRIX, synth.PATTERN_WINDOW, 10_000_000, 32, dtype)
    m = synth.crs_laplace3d(256, 256, 256, dtype)
    rng = np.random.default_rng(0x5EED)
    m.update_values(rng.uniform(0.5, 1.5, m.n_non_zero_entries()).astype(dtype))
    return m


def tile_span_histogram(m):
    off, col, _ = m.raw_parts()
    n = m.n_rows()
    starts = off[np.arange(0, n, 64)].astype(np.int64)
    keep = np.flatnonzero(np.diff(np.append(starts, off[-1])) > 0)
    lo = np.minimum.reduceat(col, starts[keep])
    hi = np.maximum.reduceat(col, starts[keep])
    span = hi.astype(np.int64) - lo + 1
    edges = [0, 1024, 4096, 16384, 65536, 262144, 1 << 20, 1 << 62]
    return "tiles by column span: " + ", ".join("<%d: %d" % (e, c) for e, c in zip(edges[1:-1] + [edges[-1]], np.histogram(span, edges)[0])).replace(
        "<%d" % edges[-1], ">=%d" % edges[-2]) + " | mean %.0f max %d" % (span.mean(), span.max())


def run(name, args, timer, out):
    dtype = np.float32
    vs = np.dtype(dtype).itemsize
    original = build(name, dtype)
    n, nnz = original.n_rows(), original.n_non_zero_entries()
    out("== %s f32: rows %d entries %d" % (name, n, nnz))
    shuffle = np.random.default_rng(0xC0FFEE).permutation(n).astype(np.uint32)
    renumbered, t_shuffle = wall_ms(lambda: original.permute_symmetric(shuffle))
    (perm, stats), t_rcm = wall_ms(renumbered.rcm)
    reordered, t_perm = wall_ms(lambda: renumbered.permute_symmetric(perm))
    mats = {"renumbered": renumbered, "reordered": reordered, "original": original}
    prep = {}
    for k, m in mats.items():
        prep[k] = m.prepare_stats("auto")[0]
    out("  rcm %.1f ms (%d components, %d levels: %.1f us per level) | permute_symmetric %.1f ms (random renumbering: %.1f ms) | "
        "prepare of the reordered matrix %.1f ms (create-time inspection included)" % (
            t_rcm, stats["n_components"], stats["n_levels"], 1e3 * t_rcm / max(1, stats["n_levels"]), t_perm, t_shuffle, prep["reordered"]))
    for k, m in mats.items():
        out("  %-10s resolves to %-8s lanes %d | span fraction %.5f | bandwidth %s | prepare %.1f ms" % (
            k, m.resolved_variant()[0], m.resolved_variant()[1], m.span_fraction(), m.bandwidth(), prep[k]))
    x, y = sm.DenseVec.zeros(n, dtype), sm.DenseVec.zeros(n, dtype)
    synth.gen_x(synth.SEED_X, n, dtype, ptr=x.data_ptr())
    t = {k: [] for k in mats}
    for _ in range(args.repeats):  # the three alternate; every round is repeated
        for k, m in mats.items():
            t[k].append(timer.ms_per_launch(lambda st, m=m: m.mvp_dev(x.data_ptr(), n, y.data_ptr(), "auto", stream=st), args.launches, args.warmup))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    for k in mats:
        out("  AUTO product, %-10s %.3f ms (%.3f .. %.3f, spread %.1f%%) | %.0f GB/s of CSR bytes" % (
            k, med[k], min(t[k]), max(t[k]), 100.0 * (max(t[k]) - min(t[k])) / med[k], (nnz * (4 + vs) + n * (4 + 2 * vs)) / med[k] / 1e6))
    gain = med["renumbered"] - med["reordered"]
    cost = t_rcm + t_perm + prep["reordered"]
    if gain > 0:
        out("  reordering has paid for itself after %.0f products: (%.1f + %.1f + %.1f) ms / (%.3f - %.3f) ms; reordered / original %.3f" % (
            cost / gain, t_rcm, t_perm, prep["reordered"], med["renumbered"], med["reordered"], med["reordered"] / med["original"]))
    else:
        out("  reordering does not pay: the reordered product is not faster (%.3f against %.3f ms)" % (med["reordered"], med["renumbered"]))
    if reordered.resolved_variant()[0] != original.resolved_variant()[0]:
        out("  the reordered matrix does not resolve as the original does:")
        out("    reordered  " + tile_span_histogram(reordered))
        out("    original   " + tile_span_histogram(original))
    # the emit pass against its byte model and the copy ceiling
    _, t_id = wall_ms(lambda: reordered.permute())
    _, t_clone = wall_ms(lambda: reordered.clone())
    emit_bytes = 2 * nnz * (4 + vs) + 12 * n
    out("  permute() with both permutations None %.1f ms, clone() %.1f ms (same create-time inspection in both); byte model of the emit "
        "pass %.2f GB (+ %.2f GB of col_perm^-1 gathers when columns are permuted) = %.2f ms at the 6.29 TB/s copy ceiling of BASELINE.md" % (
            t_id, t_clone, emit_bytes / 1e9, 4 * nnz / 1e9, emit_bytes / 6.29e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="headline,lap-varcoef")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "reorder_ab.log"))
    args = ap.parse_args()
    out = Tee(args.out)
    out("reorder_bench: launches %d warmup %d repeats %d" % (args.launches, args.warmup, args.repeats))
    timer = Timer()
    for name in args.inputs.split(","):
        run(name, args, timer, out)


if __name__ == "__main__":
    main()
