"""numpy model of the reordering operations (DESIGN.md "Reordering"), written from their definition, not from the kernels:
the reverse Cuthill-McKee ordering, row / column permutation of raw CRS arrays, the vector forms, the bandwidth and the
64-row tile-span statistic, plus the generators the reorder tests share.

A permutation is n uint32 with perm[new] = old (scipy's convention: A[perm][:, perm]).
"""
import numpy as np

# ---- graph of a square pattern ---------------------------------------------------------------------------------------
def adjacency(n, off, col):
    """u ~ v iff u != v and an entry (u, v) or (v, u) is stored (stored zeros count, duplicates once).  Returns
    (aoff[n + 1], acol) with every neighbour list ascending."""
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    keep = rows != col
    u = np.concatenate([rows[keep], col[keep]])
    v = np.concatenate([col[keep], rows[keep]])
    keys = np.unique(u * n + v) if n else np.zeros(0, np.int64)
    au, av = (keys // n, keys % n) if n else (keys, keys)
    aoff = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(au, minlength=n), out=aoff[1:])
    return aoff, av


def rcm(n, off, col):
    """The ordering of DESIGN.md: roots by smallest (degree, index) among the unvisited, levels appended in ascending
    (position of the earliest-placed parent, degree, index), the whole order reversed.
    Returns (perm uint32[n], n_components, n_levels)."""
    aoff, acol = adjacency(n, off, col)
    deg = np.diff(aoff)
    by_deg = np.lexsort((np.arange(n), deg))  # roots are tried in this order
    placed_at = np.full(n, -1, np.int64)
    order = np.zeros(n, np.int64)
    placed = comps = levels = 0
    iso = by_deg[:int(np.count_nonzero(deg == 0))]  # every isolated vertex is a root and a level of its own
    order[:len(iso)] = iso
    placed_at[iso] = np.arange(len(iso))
    placed = comps = levels = len(iso)
    rp = len(iso)
    while placed < n:
        while placed_at[by_deg[rp]] >= 0:
            rp += 1
        root = by_deg[rp]
        order[placed] = root
        placed_at[root] = placed
        fb, fe = placed, placed + 1
        placed = fe
        comps += 1
        levels += 1
        while True:
            f = order[fb:fe]
            lens = deg[f]
            tot = int(lens.sum())
            # neighbours of the frontier in frontier order: the first occurrence of a vertex carries its earliest parent
            idx = np.repeat(aoff[f] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(tot)
            nb = acol[idx]
            ppos = np.repeat(np.arange(fb, fe), lens)
            new = placed_at[nb] < 0
            nb, ppos = nb[new], ppos[new]
            if len(nb) == 0:
                break
            v, first = np.unique(nb, return_index=True)
            parent = ppos[first]
            nxt = v[np.lexsort((v, deg[v], parent))]
            order[fe:fe + len(nxt)] = nxt
            placed_at[nxt] = np.arange(fe, fe + len(nxt))
            fb, fe = fe, fe + len(nxt)
            placed = fe
            levels += 1
    return order[::-1].astype(np.uint32), comps, levels


# ---- permutation of raw CRS arrays and of vectors ----------------------------------------------------------------------
def inverse(perm):
    perm = np.asarray(perm, np.int64)
    inv = np.zeros(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    return inv.astype(np.uint32)


def permute(n_rows, n_cols, off, col, val, row_perm=None, col_perm=None):
    """out[i][j] = a[row_perm[i]][col_perm[j]]: row i of the result is row row_perm[i] of a with the same entries in the
    same storage order, every column c relabelled to col_perm^-1[c]; values untouched.  None = identity."""
    off = np.asarray(off, np.int64)
    rp = np.arange(n_rows, dtype=np.int64) if row_perm is None else np.asarray(row_perm, np.int64)
    lens = (off[1:] - off[:-1])[rp]
    out_off = np.zeros(n_rows + 1, np.int64)
    np.cumsum(lens, out=out_off[1:])
    tot = int(out_off[-1])
    src = np.repeat(off[:-1][rp] - out_off[:-1], lens) + np.arange(tot)
    out_col = np.asarray(col)[src]
    if col_perm is not None:
        out_col = inverse(col_perm)[out_col]
    return out_off.astype(np.uint32), out_col.astype(np.uint32), np.asarray(val)[src]


def permute_symmetric(n, off, col, val, perm):
    return permute(n, n, off, col, val, perm, perm)


def vec_permute(src, perm, inverse_form=False):
    """gather dst[i] = src[perm[i]]; inverse_form: scatter dst[perm[i]] = src[i]."""
    src = np.asarray(src)
    perm = np.asarray(perm, np.int64)
    if not inverse_form:
        return src[perm]
    dst = np.empty_like(src)
    dst[perm] = src
    return dst


def bandwidth(n_rows, off, col):
    """(max i - j, max j - i) over the stored entries, 0 for none."""
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(np.asarray(off, np.int64)))
    if len(rows) == 0:
        return 0, 0
    d = rows - np.asarray(col, np.int64)
    return int(max(d.max(), 0)), int(max((-d).max(), 0))


def span_fraction(n_rows, n_cols, off, col):
    """mean over the 64-row tiles that hold entries of (largest - smallest column + 1), over n_cols: the locality
    statistic AUTO tests."""
    off = np.asarray(off, np.int64)
    col = np.asarray(col, np.int64)
    n_tiles = (n_rows + 63) // 64
    if n_tiles == 0 or n_cols == 0:
        return 0.0
    t0 = off[np.minimum(np.arange(n_tiles) * 64, n_rows)]
    t1 = off[np.minimum(np.arange(1, n_tiles + 1) * 64, n_rows)]
    has = t1 > t0
    if not has.any():
        return 0.0
    lo = np.minimum.reduceat(col, t0[has])
    hi = np.maximum.reduceat(col, t0[has])
    return float((hi - lo + 1).sum()) / int(has.sum()) / n_cols


# ---- generators --------------------------------------------------------------------------------------------------------
def grid2d(nx, ny, dtype=np.float32):
    """5-point operator on an nx x ny grid, rows sorted."""
    return _stencil((nx, ny), dtype)


def grid3d(nx, ny, nz, dtype=np.float32):
    """7-point operator."""
    return _stencil((nx, ny, nz), dtype)


def _stencil(shape, dtype):
    n = int(np.prod(shape))
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    r = [idx.ravel()]
    c = [idx.ravel()]
    for ax in range(len(shape)):
        lo = [slice(None)] * len(shape)
        hi = [slice(None)] * len(shape)
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        a, b = idx[tuple(lo)].ravel(), idx[tuple(hi)].ravel()
        r += [a, b]
        c += [b, a]
    r, c = np.concatenate(r), np.concatenate(c)
    o = np.lexsort((c, r))
    r, c = r[o], c[o]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=off[1:])
    val = np.where(r == c, 2.0 * len(shape), -1.0).astype(dtype)
    return n, off.astype(np.uint32), c.astype(np.uint32), val


def from_edges(n, u, v, dtype=np.float32):
    """CRS pattern holding exactly the entries (u[k], v[k]), rows sorted."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    o = np.lexsort((v, u))
    u, v = u[o], v[o]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(u, minlength=n), out=off[1:])
    return n, off.astype(np.uint32), v.astype(np.uint32), np.arange(1, len(u) + 1).astype(dtype)


def renumber(n, off, col, val, seed):
    """the same operator with its unknowns renumbered at random: (P A P^T arrays, the permutation used)."""
    p = np.random.default_rng(seed).permutation(n).astype(np.uint32)
    o, c, v = permute_symmetric(n, off, col, val, p)
    return (o, c, v), p
