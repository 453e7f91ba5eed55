"""CPU: the numpy model of the multicolour ordering (tests/color_model.py) -- its two forms against each other, the known
answers of the definition, the properties of the colouring on every case of tests/test_color_gpu.py, and that each wrong variant
of the definition is told apart from the right one by a named case of that file."""
import numpy as np
import pytest

import color_model as cm
import reorder_model as rm
import trisolve_model as tm

NAMES = sorted(cm.CASES)
# (the big stars only add the worklist's length to star_5000: left out where the level model's row loop would take seconds)
SMALL = [n for n in NAMES if not n.startswith("worklist_grid_cap")]


def test_mix_known_answers():
    want = {0: 0, 1: 0x688990C0, 2: 0xD1132181, 3: 0x53F1E9DD, 4: 0xD97E5ED1, 0xFFFFFFFF: 0x6768824A}
    for x, h in want.items():
        assert int(cm.mix(x)) == h
    got = cm.mix(np.arange(1 << 16, dtype=np.uint32))
    assert got.dtype == np.uint32 and len(np.unique(got)) == 1 << 16  # (a bijection has no collisions)


def test_path_of_5_by_hand():
    n, off, col = cm.case("path_5")
    aoff, _ = rm.adjacency(n, off, col)
    assert cm.keys(n, aoff, 0).tolist() == [0x100000000, 0x2688990C0, 0x2D1132181, 0x253F1E9DD, 0x1D97E5ED1]
    for form in (cm.greedy, cm.jones_plassmann):
        r = form(n, off, col, 0)
        assert np.argsort(cm.keys(n, aoff, 0))[::-1].tolist() == [2, 1, 3, 4, 0]
        assert r["colors"].tolist() == [0, 1, 0, 1, 0]
        assert r["rounds"].tolist() == [2, 1, 0, 1, 2]
        assert (r["n_colors"], r["n_rounds"]) == (2, 3)
        assert r["perm"].tolist() == [0, 2, 4, 1, 3]
        assert r["color_counts"].tolist() == [3, 2]


def test_empty():
    for form in (cm.greedy, cm.jones_plassmann):
        r = form(0, np.zeros(1, np.uint32), np.zeros(0, np.uint32))
        assert (r["n_colors"], r["n_rounds"], len(r["perm"]), len(r["colors"])) == (0, 0, 0, 0)


@pytest.mark.parametrize("seed", cm.SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_the_two_forms_agree_and_the_colouring_is_greedy(name, seed):
    n, off, col = cm.case(name)
    jp = cm.expected(name, seed)
    cm.check_coloring(n, off, col, jp)
    if name.startswith("worklist_grid_cap") and seed:
        return  # (stars of a million leaves: the vertex-by-vertex form takes seconds, and seed 0 has compared the two)
    sq = cm.greedy(n, off, col, seed)
    for key in ("colors", "rounds", "perm", "color_counts"):
        assert np.array_equal(jp[key], sq[key]), key
    assert (jp["n_colors"], jp["n_rounds"]) == (sq["n_colors"], sq["n_rounds"])


def test_what_the_named_cases_come_to():
    table = {"grid_24x17": (4, (10, 11)), "grid_24x24x24": (6, (24, 22)), "grid_40x40x40": (6, (22, 23)), "chain_3000_shuffled": (3, (7, 7)),
             "isolated_5": (1, (1, 1)), "diagonal_only": (1, (1, 1)), "star_5000": (2, (2, 2)), "single": (1, (1, 1))}
    for name, (colors, rounds) in table.items():
        for seed in cm.SEEDS:
            r = cm.expected(name, seed)
            assert (r["n_colors"], r["n_rounds"]) == (colors, rounds[seed]), (name, seed)
    for k in (63, 64, 65, 130):  # a clique takes a colour per vertex, across the mask window once (65) and twice (130)
        r = cm.expected("clique_%d" % k, 0)
        assert (r["n_colors"], r["n_rounds"]) == (k, k)
    star = cm.expected("star_5000", 0)
    assert star["colors"][0] == 0 and (star["colors"][1:] == 1).all()
    # the comb: the rounds run down the path, through more than one read-back batch (4 + 8 + 16 + 32 = 60 < 70)
    comb = cm.expected("comb_70", 0)
    # (vertices 0 and 1 tie at degree 71 and the hash puts 1 first at seed 0; from there each path vertex waits for the one before
    # it, and the last one's leaf for it)
    assert comb["n_rounds"] == cm.COMB_L == 70 and comb["rounds"][1:cm.COMB_L].tolist() == list(range(cm.COMB_L - 1))
    assert cm.FIRST_BATCH * 15 < comb["n_rounds"]
    # hubs on both sides of the thread-walk limit and of the workgroup's width
    n, off, col = cm.case("hubs_around_the_thread_limit")
    assert np.diff(rm.adjacency(n, off, col)[0])[:4].tolist() == [cm.THREAD_DEG - 1, cm.THREAD_DEG, cm.THREAD_DEG + 1, 300]
    n, off, col = cm.case("hubs_around_the_block")
    assert np.diff(rm.adjacency(n, off, col)[0])[:3].tolist() == [cm.BLOCK - 1, cm.BLOCK, cm.BLOCK + 1]
    assert [cm.case("worklist_%d" % k)[0] for k in (255, 256, 257)] == [cm.BLOCK - 1, cm.BLOCK, cm.BLOCK + 1]
    assert [cm.case("worklist_grid_cap" + s)[0] for s in ("_minus_1", "", "_plus_1")] == [cm.GRID * cm.BLOCK + d for d in (-1, 0, 1)]
    n, off, col = cm.case("components_400")
    assert rm.rcm(n, off, col)[1] > 400 and (np.diff(rm.adjacency(n, off, col)[0]) == 0).sum() > 25
    assert not cm.is_pattern_symmetric(*cm.case("messy_non_symmetric"))


@pytest.mark.parametrize("name", SMALL)
def test_levels_of_the_permuted_matrix(name):
    """after permute_symmetric(perm) the triangular solves have at most n_colors levels; on a structurally symmetric pattern the
    LOWER level of a row IS its colour"""
    n, off, col = cm.case(name)
    symmetric = cm.is_pattern_symmetric(n, off, col)
    assert symmetric == (name not in ("messy_non_symmetric", "components_400"))  # (both store their entries one way only)
    for seed in cm.SEEDS:
        r = cm.expected(name, seed)
        o, c, _ = rm.permute_symmetric(n, off, col, np.zeros(len(col), np.float32), r["perm"])
        lower, n_lower = tm.levels(o, c, tm.LOWER)
        upper, n_upper = tm.levels(o, c, tm.UPPER)
        assert n_lower <= r["n_colors"] and n_upper <= r["n_colors"]
        if symmetric:
            assert n_lower == r["n_colors"] and np.array_equal(lower, r["colors"][r["perm"]])


# each wrong variant of the definition, and a named case on which the right one differs from it
TELLS = {
    "no_degree": "star_5000",        # the hub is coloured first only because of its degree
    "ascending": "comb_70",          # the rounds run UP the path, and the leaves go first
    "seed_plus_1": "grid_24x17",
    "perm_by_key": "grid_64x65",
}


@pytest.mark.parametrize("variant", sorted(TELLS))
def test_wrong_variants_are_told_apart(variant):
    assert set(TELLS) == set(cm.VARIANTS) - {"right"}
    name = TELLS[variant]
    n, off, col = cm.case(name)
    differs = []
    for seed in cm.SEEDS:
        right = cm.expected(name, seed)
        for form in (cm.greedy, cm.jones_plassmann):
            wrong = form(n, off, col, seed, variant)
            if variant == "perm_by_key":
                assert np.array_equal(wrong["colors"], right["colors"])
                differs.append(not np.array_equal(wrong["perm"], right["perm"]))
            else:
                differs.append(not np.array_equal(wrong["colors"], right["colors"]))
    assert all(differs), (variant, name, differs)
