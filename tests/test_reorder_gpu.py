"""GPU: the reverse Cuthill-McKee ordering of csrc/reorder.hip -- perm, n_components and n_levels bit for bit against the numpy
model of its definition (tests/reorder_model.py).

Switches of the level kernels, each with cases on both sides:
  * kRcmThreadDeg = 32: a frontier vertex of up to 32 neighbours is walked by one thread, a longer list by its workgroup
    (test_degree_switch: degrees 31, 32, 33, 300; the star's hub has 5000);
  * kBlock = 256 frontier vertices per workgroup of k_rcm_expand (test_level_width_switches: levels of 255, 256, 257);
  * kRcmExpandGrid * kBlock = 262144 frontier vertices per sweep of k_rcm_expand (levels of 262144 and 262145);
  * kRcmRootBlock = 1024 vertices per step of the root search (the block-diagonal case has some 400 roots among 4100 vertices)."""
import numpy as np
import pytest

import reorder_model as rm
import sparsemat_amd as sm
from sparsemat_amd import _lib

pytestmark = pytest.mark.gpu


def _check(n, off, col, val=None, dtype=np.float32, expect=None):
    val = np.ones(len(col), dtype) if val is None else val
    A = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    perm, stats = A.rcm()
    want, comps, levels = rm.rcm(n, off, col)
    assert perm.dtype == np.uint32 and len(perm) == n
    assert (stats["n_components"], stats["n_levels"]) == (comps, levels)
    assert (perm == want).all(), "first difference at %d" % int(np.argmax(perm != want))
    if expect is not None:
        assert (comps, levels) == expect
    return A, perm, stats


def _star(leaves):
    """hub 0 with `leaves` leaves: root = leaf 1, then the hub, then a level of leaves - 1 vertices"""
    return rm.from_edges(leaves + 1, np.zeros(leaves, np.int64), np.arange(1, leaves + 1))


def test_empty_and_single(gpu):
    for dtype in (np.float32, np.float64):
        A = sm.SparseMatCRS.from_raw_parts(0, 0, [0], [], np.zeros(0, dtype))
        perm, stats = A.rcm()
        assert len(perm) == 0 and stats == dict(n_components=0, n_levels=0)
        _check(1, [0, 0], [], dtype=dtype, expect=(1, 1))
        _check(1, [0, 1], [0], dtype=dtype, expect=(1, 1))  # a diagonal entry is no neighbour
    _check(5, [0, 0, 0, 0, 0, 0], [], expect=(5, 5))


@pytest.mark.parametrize("shape,levels", [((24, 17), 40), ((12, 12, 12), 34)])
def test_renumbered_grids_both_dtypes(gpu, shape, levels):
    n, off, col, val = rm._stencil(shape, np.float32)
    (off, col, val), _ = rm.renumber(n, off, col, val, seed=7)
    _, p32, _ = _check(n, off, col, val, expect=(1, levels))
    _, p64, _ = _check(n, off, col, np.random.default_rng(1).standard_normal(len(col)), dtype=np.float64)  # values never matter
    assert (p32 == p64).all()
    if len(shape) == 2:  # and the ordering does what it is for
        o, c, v = rm.permute_symmetric(n, off, col, val, p32)
        assert max(rm.bandwidth(n, o, c)) <= 18 < max(rm.bandwidth(n, off, col))


def test_path_of_3000(gpu):
    n = 3000
    ids = np.random.default_rng(3).permutation(n)  # the chain visits the vertices in this order
    _, off, col, val = rm.from_edges(n, ids[:-1], ids[1:])
    _check(n, off, col, val, expect=(1, 3000))


def test_star_with_5000_leaves(gpu):
    n, off, col, val = _star(5000)
    _, perm, _ = _check(n, off, col, val, expect=(1, 3))
    assert perm[::-1][:4].tolist() == [1, 0, 2, 3]  # all keys of the last level tie except the index


def test_degree_switch(gpu):
    """hubs of 31, 32, 33 and 300 neighbours hanging on one chain, leaves shared between neighbouring hubs"""
    u, v = [], []
    nxt = 4
    for hub, d in enumerate((31, 32, 33, 300)):
        if hub:
            u.append(hub - 1)
            v.append(hub)
        k = d - (1 if hub else 0) - (1 if hub < 3 else 0)
        u += [hub] * k
        v += list(range(nxt, nxt + k))
        nxt += k
    _, off, col, val = rm.from_edges(nxt, u, v)
    aoff, _ = rm.adjacency(nxt, off, col)
    assert np.diff(aoff)[:4].tolist() == [31, 32, 33, 300]
    _check(nxt, off, col, val)


@pytest.mark.parametrize("width", [255, 256, 257, 262144, 262145])
def test_level_width_switches(gpu, width):
    n, off, col, val = _star(width + 1)
    _check(n, off, col, val, expect=(1, 3))


def test_block_diagonal_with_isolated_and_empty_rows(gpu):
    rng = np.random.default_rng(11)
    u, v, base = [], [], 0
    for b in range(200):
        k = int(rng.integers(1, 40))
        m = int(rng.integers(k, 3 * k + 1))
        u.append(base + rng.integers(0, k, m))
        v.append(base + rng.integers(0, k, m))
        base += k
    n = base + 25  # empty rows at the end
    _, off, col, val = rm.from_edges(n, np.concatenate(u), np.concatenate(v))
    (off, col, val), _ = rm.renumber(n, off, col, val, seed=13)
    _, _, stats = _check(n, off, col, val)
    assert stats["n_components"] > 200 + 25 and stats["n_levels"] > stats["n_components"]


def test_non_symmetric_pattern_with_zeros_duplicates_and_a_diagonal(gpu):
    """random directed pattern in draw order: unsorted rows, repeated columns, diagonal entries, stored zeros"""
    rng = np.random.default_rng(19)
    n = 2500
    lens = rng.integers(0, 7, n)
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    rows = np.repeat(np.arange(n), lens)
    col = np.clip(rows + rng.integers(-40, 41, len(rows)), 0, n - 1).astype(np.uint32)
    col[::11] = rows[::11]            # diagonal entries
    col[1::13] = col[0:-1:13][:len(col[1::13])]  # repeats
    val = rng.standard_normal(len(col)).astype(np.float32)
    val[::5] = 0.0                    # stored zeros count as entries
    _, p32, _ = _check(n, off, col, val)
    _, p64, _ = _check(n, off, col, np.zeros(len(col)), dtype=np.float64)
    assert (p32 == p64).all()


def test_column_out_of_range(gpu):
    A = sm.SparseMatCRS.from_raw_parts(3, 3, [0, 1, 2, 3], [0, 5, 1], np.ones(3, np.float32), validate=False)
    with pytest.raises(sm.SparseMatPanic) as e:
        A.rcm()
    assert e.value.status == _lib.SMH_ERR_INDEX_RANGE


def test_auto_comes_back_on_the_renumbered_1024_grid(gpu):
    """1024 x 1024 5-point grid, f32: 1 048 576 rows, x = 4 MiB -- the smallest size at which AUTO's locality rule can fire.  Renumbered
    at random the matrix goes to the column-blocked / tiled family; reordered it resolves as the grid in its natural numbering
    does.  (2047 levels; the numpy model of the ordering is most of this test's time.)"""
    n, off, col, val = rm.grid2d(1024, 1024)
    natural = sm.SparseMatCRS.from_raw_parts(n, n, off, col, val)
    (so, sc, sv), _ = rm.renumber(n, off, col, val, seed=11)
    shuffled = sm.SparseMatCRS.from_raw_parts(n, n, so, sc, sv)
    assert shuffled.resolved_variant()[0] in ("colblock", "colfused", "colsplit", "tiled")
    assert shuffled.span_fraction() > 0.9
    perm, stats = shuffled.rcm()
    want, comps, levels = rm.rcm(n, so, sc)
    assert (stats["n_components"], stats["n_levels"]) == (comps, levels) == (1, 2047)
    assert (perm == want).all()
    back = shuffled.permute_symmetric(perm)
    print("variants: shuffled", shuffled.resolved_variant(), "reordered", back.resolved_variant(), "natural", natural.resolved_variant())
    print("span fraction: shuffled", shuffled.span_fraction(), "reordered", back.span_fraction(), "natural", natural.span_fraction())
    print("bandwidth: shuffled", shuffled.bandwidth(), "reordered", back.bandwidth(), "natural", natural.bandwidth())
    assert back.resolved_variant() == natural.resolved_variant()
    assert back.span_fraction() <= natural.span_fraction()
    assert max(back.bandwidth()) == 1024
