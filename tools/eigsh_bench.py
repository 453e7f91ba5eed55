#!/usr/bin/env python3
"""Ad-hoc timing of the device-resident thick-restart Lanczos eigensolver (smh_eigsh_vec, an extension) on one GPU (development aid,
not the contract bench).

Shape: the 7-point operator on g^3 with seeded NON-CONSTANT, SYMMETRIC coefficients: edge (i, i + s), s in {1, g, g^2}, carries
-(0.5 + u_s[i]) with u uniform in [0, 1), the diagonal 6.05 + u_d[i] (tools/mvp_many_bench.py's "lap-varcoef" draws every stored
value on its own and is not symmetric).  f32 and f64, LARGEST.  ONE start vector, made with numpy (default_rng(0)) and uploaded once.

What is timed (HIP events around one synchronous call; every round of both sides runs `--repeats` times after a warm-up round;
medians and min .. max):
  the body    one cycle of m bodies at columns 0 .. m-1 (restart_max = 0, no vectors) against a GMRES(m) solve of m bodies on the same
              handle, alternating, both divided by m: they share their Gram-Schmidt sweeps; the set-up is in both, GMRES's cycle end
              (one sweep over the basis) in the one and the host step in the other.
  convergence k = 4 and 8, m = 20 and 40, tol = 2^10 eps: restarts, products, n_conv, the solve's time.
  the host step   its wall time per cycle end (smh_eigsh_last_timing), beside the device time of that cycle: m = 20, 40 from the
              convergence runs, m = 128 from a run of one restart.
  the rotation    with SMH_EIGSH_TIMING set the solve waits for every rotation and reports their wall time (Yt's upload included):
              against its two models, the values moved, (ceil(l / 8) m + l + 2) n (every output tile reads the m columns again;
              l written; v_m carried: read and written), and the vector operations, 2 m l n (no FMA)."""
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
from cg_many_bench import Events  # noqa: E402


def build(g, dtype):
    m = synth.crs_laplace3d(g, g, g, dtype)
    off, col, _ = m.raw_parts()
    n = len(off) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(off.astype(np.int64)))
    col = col.astype(np.int64)
    rng = np.random.default_rng(0x5EED)
    val = np.empty(len(col), np.float64)
    diag = col == rows
    val[diag] = 6.05 + rng.random(n)[rows[diag]]
    lo, stride = np.minimum(rows, col), np.abs(rows - col)
    for s in (1, g, g * g):
        u = rng.random(n)
        pick = stride == s
        val[pick] = -(0.5 + u[lo[pick]])
    m.update_values(val.astype(dtype))
    return m


def timing():
    host, rot, cycles, rots = C.c_double(), C.c_double(), C.c_size_t(), C.c_size_t()
    check(lib().smh_eigsh_last_timing(C.byref(host), C.byref(cycles), C.byref(rot), C.byref(rots)))
    return host.value, cycles.value, rot.value, rots.value


def med(v):
    return sorted(v)[len(v) // 2]


def run(dtype, args, ev):
    m = build(args.grid, dtype)
    n, vs = m.n_rows(), np.dtype(dtype).itemsize
    m.prepare("auto")
    name = np.dtype(dtype).name
    start = sm.DenseVec.from_vec(np.random.default_rng(0).standard_normal(n).astype(dtype))
    b = sm.DenseVec.zeros(n, dtype)
    synth.gen_x(synth.SEED_X, n, dtype, ptr=b.data_ptr())
    print("== symmetric 7-point %d^3 %s: rows %d nnz %d auto=%s" % (args.grid, name, n, m.n_non_zero_entries(), m.resolved_variant()), flush=True)
    os.environ.pop("SMH_EIGSH_TIMING", None)
    # ---- the body against GMRES(m)'s -------------------------------------------------------------------------------------------
    for ncv in (20, 40):
        t_e, t_g = [], []
        for rep in range(args.repeats + 1):
            te = ev.ms(lambda: m.eigsh(4, "LA", ncv, 1e-300, 0, start, False)) / ncv
            x = sm.DenseVec.zeros(n, dtype)
            s = sm.GMRES(0.0, ncv, restart=ncv)
            tg = ev.ms(lambda: s.solve(m, b, x)) / ncv
            assert s.iterations == ncv
            if rep:
                t_e.append(te)
                t_g.append(tg)
        ratio = [a / c for a, c in zip(t_e, t_g)]
        print("    body, one cycle of m = %d: eigsh %.3f ms (%.3f .. %.3f) | GMRES(%d) %.3f ms (%.3f .. %.3f) | ratio %.3f (%.3f .. %.3f)" % (
            ncv, med(t_e), min(t_e), max(t_e), ncv, med(t_g), min(t_g), max(t_g), med(ratio), min(ratio), max(ratio)), flush=True)
    # ---- convergence, the host step, the rotation -------------------------------------------------------------------------------
    os.environ["SMH_EIGSH_TIMING"] = "1"
    for k, ncv, maxiter, tol in [(k, ncv, args.maxiter, 0.0) for k in (4, 8) for ncv in (20, 40)] + [(4, 128, 1, 1e-300)]:
        res = {}
        ms = ev.ms(lambda: res.update(r=m.eigsh(k, "LA", ncv, tol, maxiter, start, True)))
        r = res["r"]
        host, cycles, rot, rots = timing()
        l = k + (ncv - k) // 2
        restart_rots = max(rots - 1, 0)  # (the last rotation is the final one: k columns into the MultiVec)
        line = "    k = %d m = %d l = %d: n_conv %d restarts %d products %d breakdown %d | %.1f ms | host step %.3f ms per cycle end, device %.3f ms per cycle" % (
            k, ncv, l, r.n_conv, r.restarts, r.products, r.breakdown, ms, host / max(cycles, 1), (ms - host) / max(cycles, 1))
        if rots:
            # the models summed over the restarts' rotations (l columns and the carry) and the final one (k columns into the MultiVec)
            values = restart_rots * (((l + 7) // 8) * ncv + l + 2) * n + (rots - restart_rots) * (((k + 7) // 8) * ncv + (k + 3) // 4 * 4) * n
            ops = restart_rots * 2.0 * ncv * l * n + (rots - restart_rots) * 2.0 * ncv * k * n
            line += " | %d rotations %.3f ms in all (%.3f each, the final one of k columns included): %.0f GB/s by the values moved, %.0f G vector ops/s by 2 m l n" % (
                rots, rot, rot / rots, values * vs / rot / 1e6, ops / rot / 1e6)
        print(line + " | theta_0 %.6f" % r.values[0], flush=True)
        del r, res
    os.environ.pop("SMH_EIGSH_TIMING", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--maxiter", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    ev = Events()
    for dt in args.dtypes.split(","):
        run({"f32": np.float32, "f64": np.float64}[dt], args, ev)
        check(lib().smh_pool_trim())


if __name__ == "__main__":
    main()
