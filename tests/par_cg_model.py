"""numpy restatement of the row-partitioned CG (sparsemat_amd/csrc/par.hip smh_par_cg_solve_vec and the pieces at the end of
cg.hip) -- test infrastructure, not product code.  The recurrence is cg_model.cg's; what differs is WHERE the three sums of a
body are cut: every block k (rows [r0, r1), n_loc = r1 - r0) reduces its own rows to one value, the nb values meet, and every
block folds the same nb values with one workgroup (k_cg_set_rr / cg_fold_everywhere: cg_model.fold_partials from T(0)), so there
is one alpha, one beta and one stop decision.  Per block, in cg_model's trees:

  initial r.r     launch_dot(r_k, r_k, n_loc) on the block's own (16-byte aligned) buffers: device_sum(terms, reduce_blocks(n_loc), V)
  p.Ap, separate  launch_dot(p + r0, ap_k, n_loc): p is ONE full-length vector per block, the slice starts r0 elements in, so the
                  16-byte form runs iff (r0 * itemsize) % 16 == 0; else the threads stride over elements (V = 1)
  p.Ap, fused     the K1s epilogue leaves one partial per 256-row tile of the BLOCK's rows (stream_dot_partials of the slices);
                  launch_fold2: k_sum_stage1_b on reduce_blocks(tiles) workgroups, a thread striding over partials, then
                  k_reduce_stage2: device_sum(parts, reduce_blocks(tiles), 1).  (An empty block has no tile: the separate dot of
                  no terms, +0.)
  r.r of a body   k_cg_par_update on min(reduce_blocks(n_loc), 512) workgroups in the 16-byte form (r_k and ap_k are the block's
                  own allocations), cg_fold = one workgroup of k_sum_stage1 over its partials: device_sum(terms, cg_update_grid, V)

A fold of values that all started at T(0) passes a value through unchanged but for the sign of a zero, and reduce_blocks(tiles)
is 1 up to 2048 tiles where the single-matrix solver's one-workgroup fold reaches to 1024 and its two-stage fold takes the same
grid beyond: with ONE block the partitioned solver's bits are the single-matrix solver's (tests/test_par_cg_model.py).

``wrong``: names of deliberate mistakes, for the test that shows that the GPU cases can tell right from wrong
(tests/test_par_cg_model.py); never set by a test that compares with the device.
  "aligned"      an unaligned block start takes the 16-byte form
  "single_fold"  the fused partials of ALL blocks are folded in one go, as the single-matrix solver folds its own (no value per block)
  "order"        the block values are summed left to right instead of by the workgroup's tree
  "drop_last"    the last block's value is left out of every cross-block fold
  "late_stop"    the stop test comes after beta and the p sweep (x and r.r of the stopping body are complete before either
                 placement: this one shows in p alone)
  "stop_next"    ... and takes effect only when the next body has been entered
"""
import math

import numpy as np

import cg_model
import oracle
from cg_model import Result, cg_update_grid, device_sum, fold_partials, reduce_blocks, stream_dot_partials, vec_len

WRONG = ("aligned", "single_fold", "order", "drop_last", "late_stop", "stop_next")


def block_start_aligned(r0, dtype):
    return (r0 * np.dtype(dtype).itemsize) % 16 == 0


def cross_fold(vals, dtype, wrong=()):
    """every block's fold of the nb block values (one workgroup, from T(0))"""
    vals = np.array(vals, dtype)
    if "drop_last" in wrong:
        vals = vals[:-1]
    if "order" in wrong:
        return cg_model.sequential_sum(vals)
    return fold_partials(vals, False)


def fold_depth(count):
    """(additions a value passes through in a one-workgroup fold of `count` values: for the error bound of the model's own test)"""
    return (count + cg_model.K_BLOCK - 1) // cg_model.K_BLOCK + 6 + 4


def tree_depth(kind, cuts, dtype):
    """Longest chain of additions a term passes through in one of par_cg's three sums ("rr0", "pap", "pap_fused", "rr"): the
    block's own device_sum (cg_model.tree_depth; the fused dot: the tile's scan of 6 steps and 4 waves, then the two stages over
    the tile partials) and the cross-block fold."""
    V = vec_len(dtype)
    worst = 0
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        n_loc = r1 - r0
        if kind == "rr0":
            d = cg_model.tree_depth(n_loc, reduce_blocks(n_loc), V)
        elif kind == "rr":
            d = cg_model.tree_depth(n_loc, cg_update_grid(n_loc), V)
        elif kind == "pap" or n_loc == 0:
            d = cg_model.tree_depth(n_loc, reduce_blocks(n_loc), V if block_start_aligned(r0, dtype) else 1)
        else:
            tiles = (n_loc + cg_model.STREAM_TILE_ROWS - 1) // cg_model.STREAM_TILE_ROWS
            d = 1 + 6 + 4 + cg_model.tree_depth(tiles, reduce_blocks(tiles), 1)
        worst = max(worst, d)
    return worst + fold_depth(len(cuts) - 1)


class BlockSums:
    """The three sums of a body as the partitioned solver cuts them."""

    def __init__(self, cuts, dtype, fused, wrong=()):
        cuts = [int(c) for c in cuts]
        assert len(cuts) >= 2 and cuts[0] == 0 and all(a <= b for a, b in zip(cuts[:-1], cuts[1:]))
        assert set(wrong) <= set(WRONG)
        self.rows = list(zip(cuts[:-1], cuts[1:]))
        self.dtype, self.fused, self.wrong, self.V = np.dtype(dtype), fused, tuple(wrong), vec_len(dtype)

    def rr0(self, r):
        return cross_fold([device_sum(r[a:e] * r[a:e], reduce_blocks(e - a), self.V) for a, e in self.rows], self.dtype, self.wrong)

    def pap(self, p, ap):
        if self.fused and "single_fold" in self.wrong:
            parts = np.concatenate([stream_dot_partials(p[a:e], ap[a:e]) for a, e in self.rows if e > a])
            return cg_model.fold_tile_partials(parts, False)
        vals = []
        for a, e in self.rows:
            if self.fused and e > a:
                parts = stream_dot_partials(p[a:e], ap[a:e])
                vals.append(device_sum(parts, reduce_blocks(len(parts)), 1))
            else:
                V = self.V if block_start_aligned(a, self.dtype) or "aligned" in self.wrong else 1
                vals.append(device_sum(p[a:e] * ap[a:e], reduce_blocks(e - a), V))
        return cross_fold(vals, self.dtype, self.wrong)

    def rr(self, r):
        return cross_fold([device_sum(r[a:e] * r[a:e], cg_update_grid(e - a), self.V) for a, e in self.rows], self.dtype, self.wrong)


def par_cg(off, col, val, b, x0, tol, iter_max, cuts, mode="device", fused=False, product=None, wrong=()):
    """ConjugateGradient::solve (linearsolver.rs:27-61) as smh_par_cg_solve_vec carries it out on the blocks [cuts[k], cuts[k + 1]).
    fused: every block's product is the K1s kernel and leaves its p.Ap partials ("device" mode only); product: as in cg_model.cg.
    "sequential" and "wide" know no blocks: they are cg_model.cg's."""
    assert cuts[0] == 0 and cuts[-1] == len(off) - 1
    if mode != "device":
        assert not fused and not wrong
        return cg_model.cg(off, col, val, b, x0, tol, iter_max, mode=mode, product=product)
    val = np.ascontiguousarray(val)
    product = product or (lambda v: oracle.spmv(off, col, val, v))
    T = val.dtype.type
    sums = BlockSums(cuts, val.dtype, fused, wrong)
    with np.errstate(all="ignore"):  # (0 / 0 is the reference's behaviour for b = 0, not an accident)
        x = np.array(x0, val.dtype, copy=True)
        b = np.ascontiguousarray(b, val.dtype)
        r = b - product(x)                              # :38
        p = r.copy()                                    # :39
        rr = sums.rr0(r)                                # :40
        rr0, rr_list, iters, stop = rr, [], 0, False
        while iters < iter_max and not stop:
            iters += 1
            ap = product(p)                             # :43
            alpha = T(rr / sums.pap(p, ap))             # :45
            r = r - ap * alpha                          # :49
            rr_new = sums.rr(r)                         # :51
            x = x + p * alpha                           # :47 (every entered body)
            rr_old, rr = rr, rr_new
            rr_list.append(rr)
            conv = math.sqrt(float(rr)) < tol           # :52-54, before beta
            if conv and "late_stop" not in wrong and "stop_next" not in wrong:
                break
            beta = T(rr / rr_old)                       # :56
            p = p * beta + r                            # :58-59
            if conv and "late_stop" in wrong:
                break
            if conv:  # "stop_next": one more body is entered before the loop is left
                iters += 1
                ap = product(p)
                alpha = T(rr / sums.pap(p, ap))
                r = r - ap * alpha
                rr = sums.rr(r)
                x = x + p * alpha
                rr_list.append(rr)
                stop = True
    return Result(x, r, p, iters, rr, rr_list, rr0)
