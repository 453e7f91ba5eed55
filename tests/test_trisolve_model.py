"""CPU: tests/trisolve_model.py -- the numpy restatement of the level-scheduled sparse triangular solve -- is correct (against a
dense f64 solve within the bound the row depth gives, exactly on integer cases worked out by hand, on duplicates / repeated
diagonals / the other triangle, and its levels on hand cases and grids), and every matrix the GPU tests solve moves a bit under
each wrong order it can tell apart (an FMA, the chain run backwards, the products summed first)."""
import numpy as np
import pytest

import sgs_model
import trisolve_cases as tc
import trisolve_model as tm

F32, F64 = np.float32, np.float64


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def random_triangle(rng, n, density, dtype, uplo):
    rows = []
    for i in range(n):
        cand = np.arange(i) if uplo == tm.LOWER else np.arange(i + 1, n)
        pick = cand[rng.uniform(size=len(cand)) < density]
        r = [(int(c), float(rng.uniform(-1, 1))) for c in rng.permutation(pick)]
        r.insert(int(rng.integers(0, len(r) + 1)), (i, float(1.0 + len(pick) + rng.uniform())))  # diagonally dominant
        rows.append(r)
    return tm.from_rows(rows, dtype)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("uplo", [tm.LOWER, tm.UPPER])
@pytest.mark.parametrize("unit", [False, True])
def test_solve_matches_a_dense_solve_within_the_row_depth_bound(dtype, uplo, unit):
    """Substitution with d strict entries in a row commits d products, d subtractions and a division per component, so the
    computed x solves (T + E) x = b with |E| <= gamma_(d+2) |T| (Higham, Accuracy and Stability, thm 8.5), hence |x - x*| <=
    gamma_(d+2) |T^-1| |T| |x| to first order; 1.05 covers the second order.  The f64 reference solve errs by the same expression
    with f64's unit roundoff: negligible beside f32's, and for the f64 model it doubles the bound."""
    rng = np.random.default_rng(5)
    for n, density in ((1, 0.0), (17, 0.5), (60, 0.2), (90, 0.05)):
        off, col, val = random_triangle(rng, n, density, dtype, uplo)
        if unit:  # (keep |strict part| small against the implied 1)
            val = (val / (1.0 + np.abs(val).max() * n * density)).astype(dtype)
        b = rng.uniform(-1, 1, n).astype(dtype)
        x = tm.trisolve(off, col, val, b, uplo, unit)
        A = tm.dense_triangle(off, col, val, uplo, unit)
        ref = np.linalg.solve(A, b.astype(np.float64))
        d = tm.row_depth(off, col, uplo) + 2
        u = 2.0 ** (-24 if dtype == F32 else -53)
        gamma = d * u / (1 - d * u)
        bound = (1.05 if dtype == F32 else 2.1) * gamma * (np.abs(np.linalg.inv(A)) @ (np.abs(A) @ np.abs(ref)))
        assert (np.abs(x.astype(np.float64) - ref) <= bound + 1e-300).all(), (n, density, np.abs(x - ref).max(), bound.max())
        plan = tm.Plan(off, col, uplo)
        assert (bits(tm.trisolve(off, col, val, b, uplo, unit, plan=plan)) == bits(x)).all()  # the level-by-level form: same bits


HAND = [  # lower triangular, unsorted, integer-valued: every operation exact
    [(0, 2.0)],
    [(1, 4.0), (0, 1.0)],
    [(0, -3.0), (2, 1.0), (1, 2.0)],
    [(3, 2.0)],
    [(2, 5.0), (0, 1.0), (4, 8.0), (3, -1.0)],
]


@pytest.mark.parametrize("dtype", [F32, F64])
def test_solve_then_product_returns_b_exactly_on_hand_cases(dtype):
    off, col, val = tm.from_rows(HAND, dtype)
    # x chosen, b = T x by hand: row 0: 2*4 = 8; row 1: 1*4 + 4*(-2) = -4; row 2: -3*4 + 2*(-2) + 1*16 = 0; row 3: 2*0.5 = 1;
    # row 4: 5*16 + 1*4 - 1*0.5 + 8*0.25 = 85.5
    x_want = np.array([4.0, -2.0, 16.0, 0.5, 0.25], dtype)
    b = np.array([8.0, -4.0, 0.0, 1.0, 85.5], dtype)
    x = tm.trisolve(off, col, val, b, tm.LOWER, False)
    assert (bits(x) == bits(x_want)).all()
    assert (bits(tm.tri_product(off, col, val, x, tm.LOWER, False)) == bits(b)).all()
    # unit diagonal: x = [8, -4 - 8, 0 + 24 + 24, 1, 85.5 - 240 - 8 + 1]
    xu = tm.trisolve(off, col, val, b, tm.LOWER, True)
    assert xu.tolist() == [8.0, -12.0, 48.0, 1.0, -161.5]
    assert (bits(tm.tri_product(off, col, val, xu, tm.LOWER, True)) == bits(b)).all()
    # the transpose, UPPER
    o, c, v = tm.transpose(off, col, val)
    bu = tm.tri_product(o, c, v, x_want, tm.UPPER, False)
    assert (bits(tm.trisolve(o, c, v, bu, tm.UPPER, False)) == bits(x_want)).all()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_duplicates_repeated_diagonals_and_the_other_triangle(dtype):
    # duplicate off-diagonal entries are both subtracted: x1 = (10 - 2*1 - 3*1) / 5
    off, col, val = tm.from_rows([[(0, 1.0)], [(0, 2.0), (1, 5.0), (0, 3.0)]], dtype)
    assert tm.trisolve(off, col, val, np.array([1.0, 10.0], dtype), tm.LOWER, False).tolist() == [1.0, 1.0]
    # a repeated diagonal: the first is used (4, not 8), whether it comes before or after the strict entries
    off, col, val = tm.from_rows([[(0, 4.0), (0, 8.0)], [(0, 1.0), (1, 2.0), (1, 16.0)]], dtype)
    assert tm.trisolve(off, col, val, np.array([8.0, 6.0], dtype), tm.LOWER, False).tolist() == [2.0, 2.0]
    assert tm.diag_positions(off, col).tolist() == [0, 3]
    # the other triangle is ignored, in both directions
    off, col, val = tm.from_rows([[(1, 100.0), (0, 2.0)], [(0, 1.0), (1, 4.0)]], dtype)
    assert tm.trisolve(off, col, val, np.array([2.0, 9.0], dtype), tm.LOWER, False).tolist() == [1.0, 2.0]
    assert tm.trisolve(off, col, val, np.array([202.0, 8.0], dtype), tm.UPPER, False).tolist() == [1.0, 2.0]
    # no diagonal stored: an error unless the diagonal is implied
    off, col, val = tm.from_rows([[(0, 1.0)], [(0, 2.0)]], dtype)
    with pytest.raises(ValueError, match="row 1"):
        tm.trisolve(off, col, val, np.ones(2, dtype), tm.LOWER, False)
    assert tm.trisolve(off, col, val, np.ones(2, dtype), tm.LOWER, True).tolist() == [1.0, -1.0]
    # the scaled right-hand side of the SGS application: (b_i * d_i) then the solve
    off, col, val = tm.from_rows([[(0, 2.0), (1, 1.0)], [(1, 4.0)]], dtype)
    assert tm.trisolve(off, col, val, np.array([3.0, 2.0], dtype), tm.UPPER, False, scale_rhs=True).tolist() == [2.0, 2.0]


def test_levels():
    # by hand: 0 and 3 depend on nothing; 1 on 0; 2 on 0 and 1; 4 on 0, 2, 3 (lower).  Upper: no strict upper entries at all
    off, col, val = tm.from_rows(HAND, F64)
    lev, n = tm.levels(off, col, tm.LOWER)
    assert lev.tolist() == [0, 1, 2, 0, 3] and n == 4
    assert tm.levels(off, col, tm.UPPER)[0].tolist() == [0] * 5
    # a stored zero is a dependency; a duplicate counts once
    off, col, val = tm.from_rows([[(0, 1.0)], [(1, 1.0), (0, 0.0), (0, 0.0)]], F64)
    assert tm.levels(off, col, tm.LOWER)[0].tolist() == [0, 1]
    # a chain: n levels; a diagonal matrix: one; no rows: none
    off, col, val = tm.chain(37, F32)
    assert tm.levels(off, col, tm.LOWER) [1] == 37 and tm.levels(off, col, tm.LOWER)[0].tolist() == list(range(37))
    assert tm.levels(off, col, tm.UPPER)[1] == 1
    off, col, val = tm.chain(37, F32, lower=False)
    assert tm.levels(off, col, tm.UPPER)[0].tolist() == list(range(36, -1, -1))
    off, col, val = tm.from_rows([[(i, 1.0)] for i in range(9)], F64)
    assert tm.levels(off, col, tm.LOWER)[1] == 1 and tm.levels(off, col, tm.UPPER)[1] == 1
    assert tm.levels(np.zeros(1, np.uint32), np.zeros(0, np.uint32), tm.LOWER)[1] == 0
    # the five-point grid: nx + ny - 1 anti-diagonals in the natural ordering, two colours after the red-black renumbering
    off, col, val = sgs_model.lap2d(24, 17, F64)
    assert tm.levels(off, col, tm.LOWER)[1] == 40 and tm.levels(off, col, tm.UPPER)[1] == 40
    i, j = np.divmod(np.arange(24 * 17), 17)
    assert (tm.levels(off, col, tm.LOWER)[0] == i + j).all()
    o, c, v = sgs_model.permute_symmetric(off, col, val, sgs_model.red_black(24, 17))
    assert tm.levels(o, c, tm.LOWER)[1] == 2 and tm.levels(o, c, tm.UPPER)[1] == 2
    assert (tm.levels(o, c, tm.LOWER)[0] == (np.arange(408) >= 204)).all()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("uplo", [tm.LOWER, tm.UPPER])
@pytest.mark.parametrize("name", tc.NAMES)
def test_every_gpu_case_tells_the_wrong_orders_apart(name, uplo, dtype):
    """A case whose rows hold at least one strict entry can tell an FMA from two roundings; with two or more it can tell the chain
    run backwards and the products summed first.  Each such order must change the bits of x, or the GPU test's bit-for-bit
    comparison on that case would not notice it."""
    off, col, val, b = tc.system(name, dtype, uplo)
    depth = tm.row_depth(off, col, uplo)
    right = tm.trisolve(off, col, val, b, uplo, False)
    assert np.isfinite(right).all()
    wrong = (["fma"] if depth >= 1 else []) + (["backwards", "sum_first"] if depth >= 2 else [])
    assert depth >= {"one": 0, "diagonal": 0, "chain3000": 1, "switch": 1}.get(name, 2)
    for order in wrong:
        other = tm.trisolve(off, col, val, b, uplo, False, order=order)
        assert (bits(other) != bits(right)).any(), (name, uplo, order)
        assert np.allclose(other, right, rtol=1e-2 if dtype == F32 else 1e-8, atol=1e-3 if dtype == F32 else 1e-9)  # (a reordering, not another matrix)
