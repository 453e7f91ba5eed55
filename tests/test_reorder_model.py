"""CPU: the numpy model of the reverse Cuthill-McKee ordering (tests/reorder_model.py) -- its quality against scipy's
reverse_cuthill_mckee on randomly renumbered grids, and its structure on cases worked out by hand."""
import numpy as np
import pytest

import reorder_model as rm


def _bandwidth_after(n, arrays, perm):
    o, c, v = rm.permute_symmetric(n, *arrays, perm)
    return max(rm.bandwidth(n, o, c))


@pytest.mark.parametrize("name,shape", [("24x17", (24, 17)), ("300x200", (300, 200)), ("24^3", (24, 24, 24))])
def test_bandwidth_is_within_a_quarter_of_scipys(name, shape):
    """Measured: 18 / 17, 201 / 201, 444 / 444 (shuffled: 396, 59 787, 13 790).  The margin of 1.25 covers tie-breaking only."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    n, off, col, val = rm._stencil(shape, np.float32)
    arrays, _ = rm.renumber(n, off, col, val, seed=7)
    perm, comps, levels = rm.rcm(n, arrays[0], arrays[1])
    assert comps == 1 and sorted(perm.tolist()) == list(range(n))
    ours = _bandwidth_after(n, arrays, perm)
    A = sp.csr_matrix((arrays[2], arrays[1], arrays[0]), shape=(n, n))
    theirs = _bandwidth_after(n, arrays, reverse_cuthill_mckee(A, symmetric_mode=True).astype(np.uint32))
    shuffled = max(rm.bandwidth(n, arrays[0], arrays[1]))
    print(name, "levels", levels, "bandwidth shuffled", shuffled, "model", ours, "scipy", theirs)
    assert ours <= 1.25 * theirs
    assert ours < shuffled


def test_tile_span_of_the_renumbered_1024_grid_comes_back():
    """Measured: 0.992 shuffled, 0.00136 reordered, 0.00201 in the natural numbering."""
    n, off, col, val = rm.grid2d(1024, 1024)
    natural = rm.span_fraction(n, n, off, col)
    arrays, _ = rm.renumber(n, off, col, val, seed=11)
    shuffled = rm.span_fraction(n, n, arrays[0], arrays[1])
    perm, comps, levels = rm.rcm(n, arrays[0], arrays[1])
    o, c, v = rm.permute_symmetric(n, *arrays, perm)
    after = rm.span_fraction(n, n, o, c)
    print("span fraction shuffled", shuffled, "reordered", after, "natural", natural, "levels", levels)
    assert comps == 1 and levels == 2047
    assert shuffled > 0.9
    assert after <= natural


@pytest.mark.parametrize("seed", range(4))
def test_result_is_a_permutation_with_isolated_vertices_first_in_the_order(seed):
    rng = np.random.default_rng(seed)
    n = 300
    m = 260
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)  # directed, with repeats and self-loops
    u[:5] = v[:5] = np.arange(5)                          # diagonal-only rows are isolated too
    _, off, col, val = rm.from_edges(n, u, v)
    perm, comps, levels = rm.rcm(n, off, col)
    assert sorted(perm.tolist()) == list(range(n))
    aoff, _ = rm.adjacency(n, off, col)
    iso = np.flatnonzero(np.diff(aoff) == 0)
    assert len(iso) > 0
    cm = perm[::-1]  # the Cuthill-McKee order
    assert cm[:len(iso)].tolist() == iso.tolist()
    assert comps >= len(iso) and levels >= comps


def test_path_by_hand():
    # 0 - 1 - 2 - 3 - 4 stored one way only: degrees 1 2 2 2 1, root 0, one vertex per level
    n, off, col, val = rm.from_edges(5, [0, 1, 2, 3], [1, 2, 3, 4])
    perm, comps, levels = rm.rcm(n, off, col)
    assert perm.tolist() == [4, 3, 2, 1, 0] and comps == 1 and levels == 5
    # the same path numbered 2 - 0 - 3 - 1: degrees of 0..3 = 2 1 1 2, root 1 (degree 1, smaller index than 2)
    n, off, col, val = rm.from_edges(4, [2, 0, 3], [0, 3, 1])
    perm, comps, levels = rm.rcm(n, off, col)
    assert perm[::-1].tolist() == [1, 3, 0, 2] and comps == 1 and levels == 4


def test_star_by_hand():
    # hub 2, leaves 0 1 3 4: root 0 (degree 1), then the hub, then the other leaves by index (same parent, same degree)
    n, off, col, val = rm.from_edges(5, [2, 2, 2, 2, 0], [0, 1, 3, 4, 2])
    perm, comps, levels = rm.rcm(n, off, col)
    assert perm[::-1].tolist() == [0, 2, 1, 3, 4] and comps == 1 and levels == 3


def test_two_components_and_an_isolated_vertex_by_hand():
    # vertex 3 isolated (a stored diagonal does not count); component {0, 5} (degrees 1, 1); component {1, 2, 4}: 1 - 2, 1 - 4, 2 - 4
    # plus 6 hanging on 4: degrees 1:2 2:2 4:3 6:1
    n, off, col, val = rm.from_edges(7, [3, 0, 1, 1, 2, 4], [3, 5, 2, 4, 4, 6])
    perm, comps, levels = rm.rcm(n, off, col)
    # order: 3 | root 0 (deg 1, index 0), 5 | root 6 (deg 1), 4, then 1 and 2 (parent 4, degree 2 both, by index)
    assert perm[::-1].tolist() == [3, 0, 5, 6, 4, 1, 2]
    assert comps == 3 and levels == 1 + 2 + 3


def test_keys_order_a_level_by_parent_then_degree_then_index():
    # root 0 - {1, 2}; 1 - {3, 4}; 2 - {4, 5}; 5 - 6: vertex 4 has two parents and takes the earlier one (1)
    n, off, col, val = rm.from_edges(7, [0, 0, 1, 1, 2, 2, 5, 3], [1, 2, 3, 4, 4, 5, 6, 6])
    perm, comps, levels = rm.rcm(n, off, col)
    # degrees: 0:2 1:3 2:3 3:2 4:2 5:3 6:2.  roots: smallest (deg, index) = 0.  level 1: 1, 2 (parent 0; deg 3, 3).
    # level 2: parent 1 -> 3 (deg 2), 4 (deg 2); parent 2 -> 5.  level 3: 6 (parent 3).
    assert perm[::-1].tolist() == [0, 1, 2, 3, 4, 5, 6] and levels == 4


def test_permute_and_vector_forms():
    rng = np.random.default_rng(3)
    n_rows, n_cols = 6, 9
    off = np.array([0, 2, 2, 5, 6, 6, 8], np.uint32)
    col = np.array([8, 1, 4, 4, 0, 7, 2, 2], np.uint32)  # unsorted, duplicates
    val = np.arange(8, dtype=np.float32)
    rp, cp = rng.permutation(n_rows), rng.permutation(n_cols)
    o, c, v = rm.permute(n_rows, n_cols, off, col, val, rp, cp)
    dense = np.zeros((n_rows, n_cols))
    for i in range(n_rows):
        for k in range(off[i], off[i + 1]):
            dense[i, col[k]] = val[k]  # (duplicates: the last wins on both sides)
    out = np.zeros((n_rows, n_cols))
    for i in range(n_rows):
        for k in range(o[i], o[i + 1]):
            out[i, c[k]] = v[k]
    assert (out == dense[rp][:, cp]).all()
    o2, c2, v2 = rm.permute(n_rows, n_cols, o, c, v, rm.inverse(rp), rm.inverse(cp))
    assert (o2 == off).all() and (c2 == col).all() and (v2 == val).all()
    x = rng.standard_normal(n_cols)
    assert (rm.vec_permute(rm.vec_permute(x, cp), cp, True) == x).all()
    assert rm.bandwidth(n_rows, off, col) == (5 - 2, 8 - 0)
    assert rm.bandwidth(0, [0], []) == (0, 0)
