"""Host-side cost of the small host-form calls (get, apply on the values-only route, update_plan.execute) on a small matrix:
median wall time per call over a few hundred calls.  The library is whatever SPARSEMAT_HIP_LIB names."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsemat_amd as sm  # noqa: E402


def med(f, reps=400):
    for _ in range(20):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e6, ts[len(ts) // 10] * 1e6, ts[9 * len(ts) // 10] * 1e6


def main():
    rng = np.random.default_rng(3)
    n = 2000
    lengths = rng.integers(1, 9, n)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    col = np.concatenate([rng.choice(n, k, replace=False) for k in lengths]).astype(np.uint32)
    val = rng.standard_normal(len(col)).astype(np.float32)
    A = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    rows = np.repeat(np.arange(n, dtype=np.uint32), lengths)
    pick = rng.integers(0, len(col), 256)
    r, c, v = rows[pick], col[pick], rng.standard_normal(256).astype(np.float32)
    plan = A.update_plan(r, c)
    for name, f in (("get", lambda: A.get(int(r[0]), int(c[0]))),
                    ("get_many 256", lambda: A.get_many(r, c)),
                    ("apply 256 (values only)", lambda: A.apply(r, c, v)),
                    ("plan.execute 256", lambda: plan.execute(v))):
        m, lo, hi = med(f)
        print("%-26s median %8.1f us   p10 %8.1f   p90 %8.1f" % (name, m, lo, hi), flush=True)


if __name__ == "__main__":
    main()
