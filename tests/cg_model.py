"""numpy restatement of the device-resident CG (sparsemat_amd/csrc/cg.hip: kernels, driver and entry points; the reductions of
blas1.hip) and of the Jacobi-preconditioned CG (pcg.hip) -- test infrastructure, not product code.

Both recurrences are written once; HOW a reduction is carried out is a parameter (``mode``):

  "sequential"  a left-to-right fold in T from T(0): the reference's order (vector.rs:50-58) and the oracle's
  "device"      the trees as the kernels build them (below)
  "wide"        every reduction is an exact sum of the T-rounded terms' exact products (math.fsum on f64 products of f32
                data; np.longdouble for f64), rounded once to T

All other arithmetic is in T with one rounding per operation (the library is built with -ffp-contract=off and every
element-wise operation is an explicit *_rn multiply, add, subtract or divide), Ap comes from oracle.spmv (the SEQ and K1s
products are bit-exact against it) or from the caller's ``product`` (tests/test_solver_kernels_gpu.py: the device's own
product of any kernel family, checked against the oracle before it is used), so in "device" mode x, r, p, the r.r after
every body and the iteration count are the device's bit for bit.

The device's trees (kBlock = 256 threads, kWave = 64 lanes; V = 16 bytes / sizeof(T) elements per vector):
  a thread's share      vectors tid, tid + nthreads, ... (nthreads = grid * kBlock), the V elements of a vector in order,
                        then the tail element n - n % V + tid (the tail is shorter than a vector, so only threads 0..2 have
                        one); without 16-byte alignment (the VEC=false kernels) the thread strides over ELEMENTS: V = 1
  a wave                __shfl_down butterfly, offsets 32, 16, ..., 1: lane 0 ends with ((v0+v32)+(v16+v48))+... -- halving
  a workgroup           thread 0 adds the four wave sums in order, from T(0) in blas1.hip / cg.hip, from the first wave's
                        sum in pcg.hip (the two differ only in the sign of a zero)
  the partials          one workgroup: thread t folds partials t, t + 256, ... from T(0), then the same workgroup sum
Grid sizes: launch_dot uses reduce_blocks(n) (n / 2048 rounded up, at most kReducePartials = 1024); the CG update sweep the
same but at most 512; the PCG sweeps pcg_grid(n) (n / 256 rounded up, at most kPcgBlocks = 512).  The p sweeps carry no
reduction, so their grids (p_cap) cannot change a bit.  A scalar that passes through a one-value fold (k_cg_set_rr,
cg_fold_everywhere on launch_dot's result, k_pcg_alpha) goes through that fold here too.

The fused p.Ap of the K1s product (variant "stream": spmv_stream.hip / spmv_stream_xd.hip, all three kernels alike): a tile is
kStreamRows = 256 rows (one row per thread: the default, stream_rpt), thread t holds d = T(0) + round(p_r * (Ap)_r) of its
row (+0 past the last row), a wave sums its lanes by the DPP scan network (wave_sum_to_lane63: row_shr 1, 2, 4, 8 inside
each row of 16 lanes, row_bcast 15 into rows 1 and 3, row_bcast 31 into rows 2 and 3; lane 63 holds the total), thread 0
adds the four wave totals from T(0): one partial per tile.  Up to kReducePartials tiles the solver folds them with one
workgroup; beyond, k_sum_stage1 / k_pcg_sum_stage1 on reduce_blocks(tiles) workgroups (a thread strides over partials)
and then the one-workgroup fold.
"""
import math

import numpy as np

import oracle

K_BLOCK = 256
K_WAVE = 64
K_REDUCE_PARTIALS = 1024
CG_GRID_CAP = 512
K_PCG_BLOCKS = 512


def vec_len(dtype):
    return 16 // np.dtype(dtype).itemsize


def reduce_blocks(n):
    return max(1, min(K_REDUCE_PARTIALS, (n + K_BLOCK * 8 - 1) // (K_BLOCK * 8)))


def cg_update_grid(n):
    return min(reduce_blocks(n), CG_GRID_CAP)


def pcg_grid(n):
    return max(1, min(K_PCG_BLOCKS, (n + K_BLOCK - 1) // K_BLOCK))


def cg_p_grid(n, dtype):
    """k_cg_par_p's grid (no reduction in it: listed for the tests that want to know on which side of p_cap a case lies)."""
    return min(512, (n // vec_len(dtype) + K_BLOCK) // K_BLOCK)


# ---- the device's trees --------------------------------------------------------------------------------------------------
def block_sums(acc, from_first):
    """acc: [grid * 256] per-thread sums -> [grid] workgroup sums (wave butterfly, then thread 0 over the four waves)."""
    T = acc.dtype.type
    v = acc.reshape(-1, K_BLOCK // K_WAVE, K_WAVE)
    o = K_WAVE // 2
    while o:
        v = v[:, :, :o] + v[:, :, o:2 * o]  # lane l takes lane l + o; lanes >= o no longer feed lane 0
        o //= 2
    w = v[:, :, 0]
    r = w[:, 0].copy() if from_first else T(0) + w[:, 0]
    for k in range(1, K_BLOCK // K_WAVE):
        r = r + w[:, k]
    return r


def thread_sums(terms, grid, V):
    """terms: [n] in T, already rounded.  The per-thread running sums of a grid-stride sweep over V-element vectors + tail."""
    T = terms.dtype.type
    n = len(terms)
    nthreads = grid * K_BLOCK
    nv = n // V
    acc = np.zeros(nthreads, terms.dtype)
    trips = (nv + nthreads - 1) // nthreads
    if trips:
        # (padding with +0 is exact: a sum that started at +0 is never -0, and s + 0 == s bit for bit)
        body = np.zeros(trips * nthreads * V, terms.dtype)
        body[:nv * V] = terms[:nv * V]
        body = body.reshape(trips, nthreads, V)
        for k in range(trips):
            for e in range(V):
                acc = acc + body[k, :, e]
    tail = n - nv * V
    if tail:
        acc[:tail] = acc[:tail] + terms[nv * V:]
    assert acc.dtype.type is T
    return acc


def fold_partials(vals, from_first):
    """One workgroup over `vals`: thread t folds vals[t], vals[t + 256], ... from T(0); then the workgroup sum."""
    vals = np.ascontiguousarray(vals)
    return block_sums(thread_sums(vals, 1, 1), from_first)[0]


def device_sum(terms, grid, V, from_first=False):
    """Two stages: `grid` workgroups leave partials, one workgroup folds them."""
    return fold_partials(block_sums(thread_sums(terms, grid, V), from_first), from_first)


def tree_depth(n, grid, V):
    """(longest chain of additions a term passes through in device_sum, for the error bound of the model's own test)"""
    nthreads = grid * K_BLOCK
    chain = ((n // V + nthreads - 1) // nthreads) * V + 1          # a thread's run + its tail element
    chain += 6 + 4                                                 # butterfly, the four waves
    chain += (grid + K_BLOCK - 1) // K_BLOCK + 6 + 4               # the fold of the partials
    return chain


def wave_scan_lane63(v):
    """v: [B, 64] -> [B]: lane 63 after wave_sum_to_lane63 (internal.hpp).  Every step reads the OLD values of its source."""
    lane = np.arange(K_WAVE)
    for d in (1, 2, 4, 8):                               # row_shr:d within each row of 16 lanes; no source: + 0
        src = np.where(lane % 16 >= d, v[:, np.maximum(lane - d, 0)], 0).astype(v.dtype)
        v = v + src
    row = lane // 16
    for last, rows in ((15, (1, 3)), (31, (2, 3))):     # row_bcast:15 (row mask 0xA), row_bcast:31 (row mask 0xC)
        src_lane = np.where(last == 15, 16 * row - 1, 31)
        src = np.where(np.isin(row, rows), v[:, np.maximum(src_lane, 0)], 0).astype(v.dtype)
        v = v + src
    return v[:, K_WAVE - 1]


STREAM_TILE_ROWS = 256


def stream_dot_partials(p, ap):
    """The per-tile partials of p.Ap that the K1s epilogue leaves (one row per thread)."""
    T = p.dtype.type
    n = len(p)
    tiles = (n + STREAM_TILE_ROWS - 1) // STREAM_TILE_ROWS
    d = np.zeros(tiles * STREAM_TILE_ROWS, p.dtype)
    d[:n] = T(0) + p * ap
    w = wave_scan_lane63(d.reshape(-1, K_WAVE)).reshape(tiles, K_BLOCK // K_WAVE)
    t = T(0) + w[:, 0]
    for k in range(1, K_BLOCK // K_WAVE):
        t = t + w[:, k]
    return t


def fold_tile_partials(parts, from_first):
    """The single-matrix solvers' fold of the K1s partials (from_first: pcg.hip's workgroup sum)."""
    if len(parts) > K_REDUCE_PARTIALS:
        return device_sum(parts, reduce_blocks(len(parts)), 1, from_first)
    return fold_partials(parts, from_first)


def fused_pap(p, ap, from_first):
    """p.Ap as the single-matrix solvers take it from the K1s epilogue."""
    return fold_tile_partials(stream_dot_partials(p, ap), from_first)


# ---- reductions by mode --------------------------------------------------------------------------------------------------
def sequential_sum(terms):
    T = terms.dtype.type
    if len(terms) == 0:
        return T(0)
    return np.add.accumulate(np.concatenate([np.zeros(1, terms.dtype), terms]))[-1]  # (accumulate is a strict left fold)


def wide_dot(x, y):
    T = x.dtype.type
    if x.dtype == np.float32:
        return T(math.fsum((x.astype(np.float64) * y.astype(np.float64)).tolist()))  # (f32 x f32 is exact in f64)
    return T(np.sum(x.astype(np.longdouble) * y.astype(np.longdouble)))


class Reducer:
    """dot(x, y, kind): kind names the launch, which fixes grid and vector length in "device" mode:
    "dot" = launch_dot (blas1.hip), "cg_update" = cg_update_body's r.r, "pcg" = k_pcg_update's r.r and r.z."""

    def __init__(self, mode, aligned=True):
        assert mode in ("sequential", "device", "wide")
        self.mode = mode
        self.aligned = aligned  # x 16-byte aligned: the CG tail runs its VEC kernels

    def dot(self, x, y, kind):
        if self.mode == "wide":
            return wide_dot(x, y)
        terms = x * y
        if self.mode == "sequential":
            return sequential_sum(terms)
        n, V = len(x), vec_len(x.dtype)
        if kind == "dot":
            return device_sum(terms, reduce_blocks(n), V)
        if kind == "cg_update":
            return device_sum(terms, cg_update_grid(n), V if self.aligned else 1)
        assert kind == "pcg"
        return device_sum(terms, pcg_grid(n), V, from_first=True)

    def one(self, v, from_first=False):
        """a scalar that the device passes through a fold of ONE value"""
        if self.mode != "device":
            return v
        return fold_partials(np.array([v]), from_first)


class Result:
    def __init__(self, x, r, p, iterations, rr, rr_list, rr0):
        self.x, self.r, self.p, self.iterations, self.rr, self.rr_list, self.rr0 = x, r, p, iterations, rr, rr_list, rr0
        self.r_norm_squared = float(rr)  # what the solvers report: f64(T)


def diagonal(off, col, val):
    """d_i = get(i, i): the first match in storage order (sparsemat_crs.rs:54-67); 0 where there is none."""
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    n = len(off) - 1
    d = np.zeros(n, np.asarray(val).dtype)
    rows = np.repeat(np.arange(n), np.diff(off))
    hit = np.flatnonzero(col == rows)
    first = np.ones(len(hit), bool)
    first[1:] = rows[hit[1:]] != rows[hit[:-1]]
    d[rows[hit[first]]] = np.asarray(val)[hit[first]]
    return d


def cg(off, col, val, b, x0, tol, iter_max, mode="device", aligned=True, fused=False, product=None):
    """ConjugateGradient::solve (linearsolver.rs:27-61) as smh_cg_solve_vec carries it out.  aligned: x is 16-byte aligned
    (else the two tail kernels run their VEC=false forms); fused: p.Ap comes out of the K1s epilogue ("device" mode only);
    product: where A v comes from (product(v) -> A v in T; None: oracle.spmv) -- the initial residual's and every body's."""
    assert not fused or mode == "device"
    val = np.ascontiguousarray(val)
    product = product or (lambda v: oracle.spmv(off, col, val, v))
    T = val.dtype.type
    red = Reducer(mode, aligned)
    with np.errstate(all="ignore"):  # (0 / 0 is the reference's behaviour for b = 0, not an accident)
        x = np.array(x0, val.dtype, copy=True)
        b = np.ascontiguousarray(b, val.dtype)
        r = b - product(x)          # :38
        p = r.copy()                                   # :39
        rr = red.one(red.dot(r, r, "dot"))             # :40  (launch_dot, then k_cg_set_rr)
        rr0, rr_list, iters = rr, [], 0
        while iters < iter_max:
            iters += 1
            ap = product(p)         # :43
            if fused:
                pap = fused_pap(p, ap, False)
            else:
                pap = red.one(red.dot(p, ap, "dot"))   # launch_dot, folded again by every workgroup of the update
            alpha = T(rr / pap)                        # :45
            r = r - ap * alpha                         # :49
            rr_new = red.dot(r, r, "cg_update")        # :51
            x = x + p * alpha                          # :47 (every entered body)
            rr_old, rr = rr, rr_new
            rr_list.append(rr)
            if math.sqrt(float(rr)) < tol:             # :52-54, before beta
                break
            beta = T(rr / rr_old)                      # :56
            p = p * beta + r                           # :58-59
    return Result(x, r, p, iters, rr, rr_list, rr0)


def pcg(off, col, val, b, x0, tol, iter_max, mode="device", fused=False, product=None):
    """The same recurrence with z = r / diag(A) as smh_pcg_jacobi_solve carries it out (pcg.hip).  product: as in cg."""
    assert not fused or mode == "device"
    val = np.ascontiguousarray(val)
    product = product or (lambda v: oracle.spmv(off, col, val, v))
    T = val.dtype.type
    red = Reducer(mode)
    d = diagonal(off, col, val)
    with np.errstate(all="ignore"):
        x = np.array(x0, val.dtype, copy=True)
        b = np.ascontiguousarray(b, val.dtype)
        r = b - product(x)
        z = r / d
        rr = red.dot(r, r, "pcg")
        rz = red.dot(r, z, "pcg")
        p = z.copy()
        rr0, rr_list, iters = rr, [], 0
        while iters < iter_max:
            iters += 1
            ap = product(p)
            # n == 0: the driver clears the dot's result instead of launching it (the fold of one +0 is +0 either way)
            if fused:
                pap = fused_pap(p, ap, True)
            else:
                pap = red.one(red.dot(p, ap, "dot"), from_first=True)  # launch_dot, then k_pcg_alpha's fold of one value
            alpha = T(rz / pap)
            r = r - ap * alpha
            z = r / d
            rr = red.dot(r, r, "pcg")
            rz_new = red.dot(r, z, "pcg")
            x = x + p * alpha
            rr_list.append(rr)
            if math.sqrt(float(rr)) < tol:
                break
            beta = T(rz_new / rz)
            rz = rz_new
            p = p * beta + z
    return Result(x, r, p, iters, rr, rr_list, rr0)


# ---- the test matrices ---------------------------------------------------------------------------------------------------
def tridiag(n, dtype, seed=0, spread=0.0):
    """SPD tridiagonal matrix of any n: diagonal 2 + u_i, u uniform in [0.1, 1], off-diagonals -1 (strictly diagonally
    dominant), columns ascending within a row.  spread > 0: S A S with S = diag(10^v), v uniform in +-spread / 2, so that
    the diagonal varies (what a Jacobi preconditioner is for).  Returns (off, col, val)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    lens = np.full(n, 3, np.int64)
    if n:
        lens[0] -= 1
        lens[-1] -= 1
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    rows = np.repeat(i, lens)
    k = np.arange(len(rows)) - off[:-1].astype(np.int64)[rows]  # position within the row
    col = rows - 1 + k + (rows == 0)
    diag = 2.0 + rng.uniform(0.1, 1.0, n)
    val = np.where(col == rows, diag[rows], -1.0)
    if spread:
        s = 10.0 ** rng.uniform(-spread / 2, spread / 2, n)
        val = val * s[rows] * s[col]
    return off, col.astype(np.uint32), val.astype(dtype)
