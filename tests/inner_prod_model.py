"""numpy restatement of the three device routes of SparseMatrix::inner_prod, lhs^T (A rhs) (spmv_inner_prod in
sparsemat_amd/csrc/spmv_dispatch.hip) -- test infrastructure, not product code.  The trees that the BLAS-1 kernels and the K1s
epilogue share with the solvers are tests/cg_model.py's; only what inner_prod adds is written here.  All arithmetic is in T with one
rounding per operation (the library is built with -ffp-contract=off); `fma` is an exactly rounded fused multiply-add (K1r's r2_fma).

  fold2          launch_fold2 (blas1.hip): k_sum_stage1_b on reduce_blocks(count) workgroups -- thread i of the grid folds in[i],
                 in[i + grid * 256], ... from T(0), the wave butterfly, thread 0 over the four waves from T(0) -- then
                 k_reduce_stage2, one workgroup over the partials in the same way: two workgroups in the first stage from 2049
                 partials on.  (The solvers' fold of the K1s partials, cg_model.fold_tile_partials, is ONE workgroup up to 1024
                 partials and these two stages beyond; up to 2048 the first stage is that one workgroup and the second folds a
                 single value, so the two give the same bits at every count -- a one-workgroup fold kept beyond 2048 does not.)
  stream_route   K1s, K1s XS, XD and XD-V with y == NULL: thread t of a tile holds d = T(0) + round(lhs_r * y_r) of its row
                 (rows_per_thread == 2, the SMH_STREAM_RPT tuning knob: rows t and t + 256 of a 512-row tile, one after the other),
                 the DPP scan network, four waves from T(0): one partial per tile (cg_model.stream_dot_partials); fold2.
  generic_route  every kernel without a dot form: y = A rhs, then launch_dot(lhs, y).
  ring_route     K1r's DOT form (k_spmv_ring2<..., DOT = true>, spmv_ring2.hip); see there.

A row WITHOUT entries is no term in any route (the reference reads lhs[i] inside the entry loop, sparsematrix.rs:161-171).  With
finite lhs that changes no bit -- every accumulator starts at +0 and never holds -0, and lhs_i * (+0) = +-0 added to it leaves it --
so the models multiply every row; a caller with non-finite lhs on empty rows passes `zero_empty_rows(lhs, off)`."""
import numpy as np

import cg_model as cm
import oracle

F32, F64 = np.float32, np.float64


# ---- an exactly rounded fused multiply-add ---------------------------------------------------------------------------------------
def _two_sum(a, b):
    """s = round(a + b) and e with a + b == s + e exactly (Knuth)"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """p = round(a * b) and e with a * b == p + e exactly (Veltkamp's split, Dekker's product; no underflow of e in these tests)"""
    c = a.dtype.type(2 ** 27 + 1)
    p = a * b
    t = a * c
    ah = t - (t - a)
    al = a - ah
    t = b * c
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_to_odd(a, b):
    """a + b rounded to odd: exact where it is representable, else the neighbour whose last mantissa bit is set"""
    s, e = _two_sum(a, b)
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    toward = np.where(e > 0, np.inf, -np.inf)
    return np.where((e != 0) & even, np.nextafter(s, toward), s)


def fma(a, b, c):
    """round(a * b + c), ONE rounding, elementwise in the arrays' type (finite data in the normal range).
    f32: a * b is exact in f64; the sum is rounded to odd at 53 bits, after which the rounding to 24 bits is the exact result's
    (53 >= 24 + 2).  f64: a * b = p + e exactly, (th, tl) = c + p exactly, v = tl + e rounded to odd, round(th + v) (Boldo and
    Melquiond, Emulation of a FMA and correctly rounded sums: proved algorithms using rounding to odd, 2008).  Where the product is
    an exact zero the result is c + (+-0), where c is zero it is round(a * b): IEEE's rules for the signs of zeros."""
    a, b, c = np.broadcast_arrays(np.asarray(a), np.asarray(b), np.asarray(c))
    T = a.dtype
    assert T == b.dtype == c.dtype and T in (np.dtype(F32), np.dtype(F64))
    with np.errstate(all="ignore"):
        if T == np.dtype(F32):
            general = _add_to_odd(a.astype(F64) * b.astype(F64), c.astype(F64)).astype(F32)
        else:
            p, e = _two_prod(a, b)
            th, tl = _two_sum(c, p)
            general = th + _add_to_odd(tl, e)
        plain = a * b
        return np.where((a == 0) | (b == 0), c + plain, np.where(c == 0, plain, general)).astype(T)


# ---- what the routes share -------------------------------------------------------------------------------------------------------
def pad_lhs(lhs, n_rows):
    """inner_prod_dev continues a short (but legal) lhs with zeros"""
    lhs = np.ascontiguousarray(lhs)
    assert len(lhs) <= n_rows
    out = np.zeros(n_rows, lhs.dtype)
    out[:len(lhs)] = lhs
    return out


def zero_empty_rows(lhs, off):
    """lhs continued to n_rows and with +0 on the rows without entries: what the device makes of them"""
    n_rows = len(off) - 1
    out = pad_lhs(lhs, n_rows)
    out[np.diff(np.asarray(off).astype(np.int64)) == 0] = 0
    return out


def fold2(parts):
    parts = np.ascontiguousarray(parts)
    return cm.device_sum(parts, cm.reduce_blocks(len(parts)), 1, from_first=False)


def fold2_depth(count):
    """(longest chain of additions a partial passes through in fold2)"""
    return cm.tree_depth(count, cm.reduce_blocks(count), 1)


# ---- K1s -------------------------------------------------------------------------------------------------------------------------
def stream_partials(lhs, y, rows_per_thread=1):
    """the epilogue's partials, one per tile of 256 * rows_per_thread rows"""
    if rows_per_thread == 1:
        return cm.stream_dot_partials(lhs, y)
    T = lhs.dtype.type
    n, tile = len(lhs), cm.STREAM_TILE_ROWS * rows_per_thread
    tiles = (n + tile - 1) // tile
    terms = np.zeros(tiles * tile, lhs.dtype)
    terms[:n] = lhs * y
    terms = terms.reshape(tiles, rows_per_thread, cm.STREAM_TILE_ROWS)  # thread t: rows t, t + 256, ... of its tile
    d = np.zeros((tiles, cm.STREAM_TILE_ROWS), lhs.dtype)
    for rr in range(rows_per_thread):
        d = d + terms[:, rr, :]
    w = cm.wave_scan_lane63(d.reshape(-1, cm.K_WAVE)).reshape(tiles, cm.K_BLOCK // cm.K_WAVE)
    t = T(0) + w[:, 0]
    for k in range(1, cm.K_BLOCK // cm.K_WAVE):
        t = t + w[:, k]
    return t


def stream_route(lhs, y, rows_per_thread=1):
    """y: the storage-order product (oracle.spmv), which K1s gives bit for bit"""
    y = np.ascontiguousarray(y)
    return fold2(stream_partials(pad_lhs(lhs, len(y)), y, rows_per_thread))


# ---- every kernel without a dot form ---------------------------------------------------------------------------------------------
def generic_route(lhs, y):
    """launch_dot over the T-rounded products lhs_i * y_i: reduce_blocks(n_rows) workgroups, a thread over vectors of 16 bytes.
    The VEC = false form of k_dot_stage1 (a thread strides over elements) runs when one of the two buffers is not 16-byte aligned;
    the tests cannot reach it through inner_prod: y is the handle's staging buffer, lhs the storage a DenseVec allocated, the scratch
    copy of the host entry point or the zero-continued copy of a short lhs -- each the start of a device allocation, which is
    256-byte aligned.  (Only a DenseVec wrapped around a caller's own misaligned pointer would take it; its order is V = 1.)"""
    y = np.ascontiguousarray(y)
    terms = pad_lhs(lhs, len(y)) * y
    return cm.device_sum(terms, cm.reduce_blocks(len(y)), cm.vec_len(y.dtype))


# ---- K1r's DOT form --------------------------------------------------------------------------------------------------------------
RING_WRONG = ("ru_double", "ru_half", "waves_other", "waves_reversed", "units_descending", "muladd", "no_tail", "tail_lhs_val_first",
              "plan_order_slots")


def ring_geometry(lanes, dtype, ring_entries):
    """(rows per unit, wavefronts per workgroup): RU = SB * (64 / lanes) with SB = min(lanes, kRing2SB = 2) for f32 and
    min(lanes, SMH_RING2_SB64 = 1) for f64; Ring2Cfg::kThreads = 1024 when the ring takes more than 64 KiB, else 512"""
    size = np.dtype(dtype).itemsize
    sb = min(lanes, 2 if size == 4 else 1)
    threads = 1024 if ring_entries * size > 65536 else 512
    return sb * (64 // lanes), threads // 64


def ring_slot_block(slot, n_blocks):
    """the plan's row range that the workgroup with blockIdx.x == slot takes (the XCD-aware order of k_spmv_ring2: workgroups
    8 k + g, which share XCD g's L2, take the contiguous ranges g * n_blocks / 8 + k); the partial stays in slot blockIdx.x"""
    assert n_blocks % 8 == 0  # (ensure_ring_plan rounds the number of row ranges up to a multiple of 8: the grid is the plan)
    return (slot & 7) * (n_blocks // 8) + (slot >> 3)


def ring_block_partial(lhs, y_ring, block_phases, ru, n_waves, wrong=()):
    """one workgroup: its phases in order; row r of a phase [rb, re) is kept by lane (r - rb) % RU of wave ((r - rb) // RU) % n_waves,
    which adds fma(lhs[r], y_ring[r], .) to its accumulator, its units in ascending order; then the halving butterfly to lane 0 and
    the waves in index order from T(0)"""
    T = y_ring.dtype.type
    dacc = np.zeros((n_waves, cm.K_WAVE), y_ring.dtype)
    for rb, re in block_phases:
        rb, re = int(rb), int(re)
        per_round = n_waves * ru                           # rows of one unit of every wave
        rounds = range((re - rb + per_round - 1) // per_round)
        for k in (reversed(rounds) if "units_descending" in wrong else rounds):
            r0 = rb + k * per_round
            r1 = min(re, r0 + per_round)
            i = np.arange(r1 - r0)
            w, lane = i // ru, i % ru
            if "muladd" in wrong:
                dacc[w, lane] = dacc[w, lane] + lhs[r0:r1] * y_ring[r0:r1]
            else:
                dacc[w, lane] = fma(lhs[r0:r1], y_ring[r0:r1], dacc[w, lane])
    o = cm.K_WAVE // 2
    while o:
        dacc = dacc[:, :o] + dacc[:, o:2 * o]
        o //= 2
    t = T(0)
    for w in (reversed(range(n_waves)) if "waves_reversed" in wrong else range(n_waves)):
        t = t + dacc[w, 0]
    return t


def ring_partials(lhs, y_ring, phase_ptr, phases, lanes, dtype, ring_entries, tail=None, wrong=()):
    """the n_blocks + 1 partials launch_fold2 is given.  phases: [n, >= 2] rows (row_begin, row_end, ...) as SparseMatCRS.ring_plan()
    reports them; y_ring: the row sums as the ring phases leave them (ring_sums); tail: ring_sums' too.  wrong: names from RING_WRONG
    -- only for showing that a test case tells them apart."""
    assert set(wrong) <= set(RING_WRONG)
    y_ring = np.ascontiguousarray(y_ring, dtype)
    T = y_ring.dtype.type
    lhs = pad_lhs(np.ascontiguousarray(lhs, dtype), len(y_ring))
    ru, n_waves = ring_geometry(lanes, dtype, ring_entries)
    if "ru_double" in wrong:
        ru *= 2
    if "ru_half" in wrong:
        ru = max(1, ru // 2)
    if "waves_other" in wrong:
        n_waves = 24 - n_waves  # (8 <-> 16)
    n_blocks = len(phase_ptr) - 1
    parts = np.zeros(n_blocks + 1, dtype)  # (the launch clears them: a row range without phases leaves +0)
    for slot in range(n_blocks):
        b = slot if "plan_order_slots" in wrong else ring_slot_block(slot, n_blocks)
        p0, p1 = int(phase_ptr[b]), int(phase_ptr[b + 1])
        if p1 > p0:
            parts[slot] = ring_block_partial(lhs, y_ring, [(ph[0], ph[1]) for ph in phases[p0:p1]], ru, n_waves, wrong)
    if tail is not None and "no_tail" not in wrong:
        acc = T(0)
        for r, v, xv in zip(*tail):  # k_ring2_tail_dot: one thread, storage order
            if "tail_lhs_val_first" in wrong:
                acc = fma(T(lhs[r] * v), xv, acc)[()]
            else:
                acc = fma(lhs[r], T(v * xv), acc)[()]
        parts[n_blocks] = acc
    return parts


def ring_route(lhs, y_ring, phase_ptr, phases, lanes, dtype, ring_entries, tail=None, wrong=()):
    return fold2(ring_partials(lhs, y_ring, phase_ptr, phases, lanes, dtype, ring_entries, tail, wrong))


def ring_sums(off, col, val, x, lanes, borrowed):
    """(y_ring, tail) of a handle's K1r launch.  Owned arrays are padded to whole 16-byte chunks: the ring phases sum every entry in
    the lane-group order (oracle.spmv_lanes) and there is no tail.  Borrowed arrays that end inside a chunk (nnz % 4 != 0): the ring
    phases touch the entries below nnz & ~3 only -- the lane-group sums of the arrays cut off there (the chunk grid is anchored at
    entry 0, so cutting moves nothing) -- and the last nnz % 4 entries go to k_ring2_tail_dot as tail = (rows, values, x[columns])."""
    off = np.asarray(off)
    nnz = int(off[-1])
    limit = (nnz & ~3) if borrowed else nnz
    if limit == nnz:
        return oracle.spmv_lanes(off, col, val, x, lanes), None
    if limit == 0:
        y = np.zeros(len(off) - 1, val.dtype)  # (no ring launch at all)
    else:
        y = oracle.spmv_lanes(np.minimum(off, limit).astype(np.uint32), col[:limit], val[:limit], x, lanes)
    k = np.arange(limit, nnz)
    rows = np.searchsorted(off.astype(np.int64), k, side="right") - 1  # the row with off[r] <= k < off[r + 1]
    return y, (rows, val[limit:], x[col[limit:]])


def ring_depth(phase_ptr, phases, lanes, dtype, ring_entries, n_tail=0):
    """(longest chain of roundings a term passes through in ring_route, not counting those inside y_ring)"""
    ru, n_waves = ring_geometry(lanes, dtype, ring_entries)
    n_blocks = len(phase_ptr) - 1
    most = 0
    for b in range(n_blocks):
        chain = 0
        for ph in phases[int(phase_ptr[b]):int(phase_ptr[b + 1])]:
            units = (int(ph[1]) - int(ph[0]) + ru - 1) // ru
            chain += (units + n_waves - 1) // n_waves  # a lane's fmas in this phase
        most = max(most, chain)
    return max(most, n_tail + 1) + 6 + n_waves + fold2_depth(n_blocks + 1)


# ---- the single-window phase plan (build_ring_plan, spmv_ring.hip), for the tests that have no device ----------------------------
def ring_plan_rows(off, col, n_blocks, ring_entries):
    """(phase_ptr, phases[n, 3] = (row_begin, row_end, use_ring)) of the single-window plan: per 64-row tile the span of its columns
    (k_tile_span), a row range of ceil(tiles / n_blocks) tiles per workgroup, a phase = as many consecutive tiles as keep the union
    of their spans within the ring; runs of tiles wider than the ring make a gather phase (use_ring 0)."""
    off = np.asarray(off).astype(np.int64)
    col = np.asarray(col).astype(np.int64)
    n_rows = len(off) - 1
    n_tiles = (n_rows + 63) // 64
    tile_off = off[np.minimum(np.arange(n_tiles + 1) * 64, n_rows)]
    cmin = np.array([col[a:b].min() if b > a else 1 for a, b in zip(tile_off[:-1], tile_off[1:])], np.int64)
    cmax = np.array([col[a:b].max() if b > a else 0 for a, b in zip(tile_off[:-1], tile_off[1:])], np.int64)
    per_block = (n_tiles + n_blocks - 1) // n_blocks if n_blocks else 0
    phase_ptr, phases = np.zeros(n_blocks + 1, np.uint32), []
    for b in range(n_blocks):
        phase_ptr[b] = len(phases)
        t = min(b * per_block, n_tiles)
        t_end = min(t + per_block, n_tiles)
        while t < t_end:
            e = t + 1
            empty0 = cmin[t] > cmax[t]
            if not empty0 and cmax[t] + 1 - cmin[t] > ring_entries:
                while e < t_end and cmin[e] <= cmax[e] and cmax[e] + 1 - cmin[e] > ring_entries:
                    e += 1
                phases.append((t * 64, min(e * 64, n_rows), 0))
                t = e
                continue
            umin, umax, some = cmin[t], cmax[t], not empty0
            while e < t_end:
                if cmin[e] > cmax[e]:
                    e += 1
                    continue
                nmin = min(umin, cmin[e]) if some else cmin[e]
                nmax = max(umax, cmax[e]) if some else cmax[e]
                if nmax + 1 - nmin > ring_entries:
                    break
                umin, umax, some = nmin, nmax, True
                e += 1
            phases.append((t * 64, min(e * 64, n_rows), 1))
            t = e
    phase_ptr[n_blocks] = len(phases)
    return phase_ptr, np.array(phases, np.uint32).reshape(-1, 3)
