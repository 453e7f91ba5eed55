"""numpy model of the multicolour ordering (DESIGN.md "Multicolour ordering", smh_crs_color), written from its definition, not
from the kernels -- twice: ``greedy`` is sequential greedy over the sorted keys, ``jones_plassmann`` the synchronous rounds -- plus
the cases tests/test_color_gpu.py and tests/test_color_model.py share.

Definition.  The graph is the ordering's (reorder_model.adjacency).  h(v) = mix(v XOR seed) on 32 bits; the priority of v is
the 64-bit key deg(v) << 32 | h(v), all keys distinct.  Visiting the vertices in DESCENDING key order, each takes the smallest
colour >= 0 that no neighbour of higher key holds.  round(v) = 0 when no neighbour has a higher key, else 1 + max round(w) over
the neighbours w of higher key.  perm[new] = old is the vertices sorted by (colour, index).

``variant`` names the wrong definitions a test must be able to tell from the right one: "no_degree" (the key is the hash alone),
"ascending" (the smallest key first), "seed_plus_1", "perm_by_key" (perm sorted by (colour, key))."""
import numpy as np

import reorder_model as rm

VARIANTS = ("right", "no_degree", "ascending", "seed_plus_1", "perm_by_key")


def mix(x):
    """the 32-bit bijection of the definition, on an array (or a scalar) of uint32"""
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    x = x ^ (x >> np.uint64(16))
    return x.astype(np.uint32)


def keys(n, aoff, seed, variant="right"):
    """the priorities as uint64; the vertex visited first has the LARGEST one (every variant is brought to that form)"""
    assert variant in VARIANTS
    deg = np.diff(aoff).astype(np.uint64)
    s = (seed + 1 if variant == "seed_plus_1" else seed) & 0xFFFFFFFF
    h = mix(np.arange(n, dtype=np.uint64) ^ np.uint64(s)).astype(np.uint64)
    k = h if variant == "no_degree" else (deg << np.uint64(32)) | h
    return ~k if variant == "ascending" else k


def _perm(colors, key, variant):
    n = len(colors)
    if variant == "perm_by_key":
        return np.lexsort((key, colors)).astype(np.uint32)
    return np.lexsort((np.arange(n), colors)).astype(np.uint32)


def _result(colors, rounds, key, variant):
    n = len(colors)
    colors = np.asarray(colors, np.uint32)
    return dict(colors=colors, rounds=np.asarray(rounds, np.uint32), perm=_perm(colors, key, variant),
                n_colors=int(colors.max()) + 1 if n else 0, n_rounds=int(np.max(rounds)) + 1 if n else 0,
                color_counts=np.bincount(colors, minlength=1 if n else 0) if n else np.zeros(0, np.int64))


def greedy(n, off, col, seed=0, variant="right"):
    """Sequential greedy over the keys in descending order: when v is visited, its coloured neighbours are exactly those of
    higher key.  The rounds come from their recursive definition in the same sweep."""
    aoff, acol = rm.adjacency(n, off, col)
    key = keys(n, aoff, seed, variant)
    order = np.argsort(key, kind="stable")[::-1].tolist()
    ao, ac = aoff.tolist(), acol.tolist()
    colors, rounds = [-1] * n, [0] * n
    for v in order:
        used, rd = set(), 0
        for w in ac[ao[v]:ao[v + 1]]:
            if colors[w] >= 0:
                used.add(colors[w])
                if rounds[w] + 1 > rd:
                    rd = rounds[w] + 1
        c = 0
        while c in used:
            c += 1
        colors[v], rounds[v] = c, rd
    return _result(colors, rounds, key, variant)


def jones_plassmann(n, off, col, seed=0, variant="right"):
    """Synchronous rounds: round k colours every uncoloured vertex whose higher-key neighbours were all coloured BEFORE round k,
    each with the smallest colour none of them holds."""
    aoff, acol = rm.adjacency(n, off, col)
    key = keys(n, aoff, seed, variant)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(aoff))
    up = key[acol] > key[src]
    src, dst = src[up], acol[up]  # v -> each neighbour of higher key
    colors = np.full(n, -1, np.int64)
    rounds = np.zeros(n, np.int64)
    k = 0
    while (colors < 0).any():
        waiting = np.bincount(src, weights=(colors[dst] < 0), minlength=n) > 0
        ready = (colors < 0) & ~waiting
        assert ready.any()
        e = ready[src]
        pairs = np.unique(src[e] * (n + 1) + colors[dst[e]])  # (vertex, colour of a higher neighbour), ascending
        pv, pc = pairs // (n + 1), pairs % (n + 1)
        start = np.searchsorted(pv, pv)  # where each vertex's run begins
        rank = np.arange(len(pv)) - start
        free = np.bincount(pv, minlength=n).astype(np.int64)  # all of 0 .. m-1 taken: the answer is m
        gap = pc != rank  # the first position where the colours skip one is the smallest free colour
        np.minimum.at(free, pv[gap], rank[gap])
        colors[ready] = free[ready]
        rounds[ready] = k
        k += 1
    return _result(colors, rounds, key, variant)


def check_coloring(n, off, col, res):
    """proper on the symmetrised graph; n_colors <= max deg + 1; a vertex of colour c > 0 has a neighbour of every colour
    below c; perm is the stable sort by colour"""
    aoff, acol = rm.adjacency(n, off, col)
    colors = res["colors"].astype(np.int64)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(aoff))
    assert (colors[src] != colors[acol]).all()
    deg = np.diff(aoff)
    assert res["n_colors"] <= (int(deg.max()) + 1 if n else 0)
    below = colors[acol] < colors[src]
    distinct_below = len(np.unique(src[below] * (n + 1) + colors[acol[below]]))
    assert distinct_below == int(colors.sum())
    assert (res["perm"] == np.argsort(colors, kind="stable")).all()
    assert int(res["color_counts"].sum()) == n


def is_pattern_symmetric(n, off, col):
    off = np.asarray(off, np.int64)
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    c = np.asarray(col, np.int64)
    a = np.unique(r * n + c) if n else np.zeros(0, np.int64)
    b = np.unique(c * n + r) if n else np.zeros(0, np.int64)
    return len(a) == len(b) and bool((a == b).all())


# ---- the cases ---------------------------------------------------------------------------------------------------------
# the constants of csrc/color.hip the cases are built around
THREAD_DEG = 32      # kColorThreadDeg
BLOCK = 256          # kColorBlock
WINDOW = 64          # kColorWindow
GRID = 4096          # kColorGrid
FIRST_BATCH = 4      # kColorFirstBatch


def symmetric_edges(n, u, v):
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    return rm.from_edges(n, np.concatenate([u, v]), np.concatenate([v, u]))[:3]


def path(n, shuffle_seed=None):
    ids = np.arange(n) if shuffle_seed is None else np.random.default_rng(shuffle_seed).permutation(n)
    return symmetric_edges(n, ids[:-1], ids[1:])


def star(leaves):
    return symmetric_edges(leaves + 1, np.zeros(leaves, np.int64), np.arange(1, leaves + 1))


def hubs(degrees):
    """hubs 0 .. len - 1 of the given degrees on one chain, each with leaves of its own"""
    u, v, nxt = [], [], len(degrees)
    for hub, d in enumerate(degrees):
        if hub:
            u.append(hub - 1)
            v.append(hub)
        k = d - (1 if hub else 0) - (1 if hub < len(degrees) - 1 else 0)
        u += [hub] * k
        v += list(range(nxt, nxt + k))
        nxt += k
    return symmetric_edges(nxt, u, v)


def clique(k):
    i, j = np.divmod(np.arange(k * k), k)
    keep = i != j
    return rm.from_edges(k, i[keep], j[keep])[:3]


def comb(L):
    """a path of L vertices where vertex i carries L - i pendant leaves: degrees fall along the path, so the rounds run down it"""
    u, v, nxt = list(range(L - 1)), list(range(1, L)), L
    for i in range(L):
        u += [i] * (L - i)
        v += list(range(nxt, nxt + L - i))
        nxt += L - i
    return symmetric_edges(nxt, u, v)


def components():
    """some 400 components of 1 .. 39 vertices, isolated vertices and empty rows among them, renumbered at random"""
    rng = np.random.default_rng(11)
    u, v, base = [], [], 0
    for b in range(400):
        k = int(rng.integers(1, 40))
        m = int(rng.integers(k, 3 * k + 1))
        u.append(base + rng.integers(0, k, m))
        v.append(base + rng.integers(0, k, m))
        base += k
    n = base + 25
    _, off, col, val = rm.from_edges(n, np.concatenate(u), np.concatenate(v))
    (off, col, val), _ = rm.renumber(n, off, col, val, seed=13)
    return n, off, col


def messy():
    """a random directed pattern in draw order: unsorted rows, repeated columns, diagonal entries (stored zeros are the test's)"""
    rng = np.random.default_rng(19)
    n = 2500
    lens = rng.integers(0, 7, n)
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    rows = np.repeat(np.arange(n), lens)
    col = np.clip(rows + rng.integers(-40, 41, len(rows)), 0, n - 1).astype(np.uint32)
    col[::11] = rows[::11]
    col[1::13] = col[0:-1:13][:len(col[1::13])]
    return n, off, col


def grid(shape, renumber_seed=None):
    n, off, col, val = rm._stencil(shape, np.float32)
    if renumber_seed is not None:
        (off, col, val), _ = rm.renumber(n, off, col, val, seed=renumber_seed)
    return n, off, col


GRIDS = {
    "grid_24x17": lambda: grid((24, 17)),
    "grid_24x17_renumbered": lambda: grid((24, 17), 7),
    "grid_64x65": lambda: grid((64, 65)),
    "grid_64x65_renumbered": lambda: grid((64, 65), 8),
    "grid_24x24x24": lambda: grid((24, 24, 24)),
    "grid_24x24x24_renumbered": lambda: grid((24, 24, 24), 9),
    "grid_40x40x40": lambda: grid((40, 40, 40)),
}
COMB_L = 70  # 70 rounds at seed 0: batches of 4, 8, 16, 32 rounds and six rounds of a fifth
CASES = dict(GRIDS)
CASES.update({
    "single": lambda: (1, np.zeros(2, np.uint32), np.zeros(0, np.uint32)),
    "single_with_diagonal": lambda: (1, np.array([0, 1], np.uint32), np.zeros(1, np.uint32)),
    "diagonal_only": lambda: (6, np.arange(7, dtype=np.uint32), np.arange(6, dtype=np.uint32)),
    "isolated_5": lambda: (5, np.zeros(6, np.uint32), np.zeros(0, np.uint32)),
    "path_5": lambda: path(5),
    "chain_3000_shuffled": lambda: path(3000, 3),
    "star_5000": lambda: star(5000),
    "hubs_around_the_thread_limit": lambda: hubs((THREAD_DEG - 1, THREAD_DEG, THREAD_DEG + 1, 300)),
    "hubs_around_the_block": lambda: hubs((BLOCK - 1, BLOCK, BLOCK + 1)),
    "clique_63": lambda: clique(63),
    "clique_64": lambda: clique(64),
    "clique_65": lambda: clique(65),
    "clique_130": lambda: clique(130),
    "comb_70": lambda: comb(COMB_L),
    "components_400": components,
    "messy_non_symmetric": messy,
    "worklist_255": lambda: path(BLOCK - 1, 5),
    "worklist_256": lambda: path(BLOCK, 5),
    "worklist_257": lambda: path(BLOCK + 1, 5),
    "worklist_grid_cap_minus_1": lambda: star(GRID * BLOCK - 2),
    "worklist_grid_cap": lambda: star(GRID * BLOCK - 1),
    "worklist_grid_cap_plus_1": lambda: star(GRID * BLOCK),
})
SEEDS = (0, 1)

_CACHE = {}


def case(name):
    """(n, off, col) of a named case, built once"""
    if name not in _CACHE:
        n, off, col = CASES[name]()
        _CACHE[name] = (n, np.asarray(off, np.uint32), np.asarray(col, np.uint32))
    return _CACHE[name]


_EXPECTED = {}


def expected(name, seed):
    """the model's result for a named case (the round form: the quicker one), computed once and shared"""
    if (name, seed) not in _EXPECTED:
        _EXPECTED[name, seed] = jones_plassmann(*case(name), seed=seed)
    return _EXPECTED[name, seed]
