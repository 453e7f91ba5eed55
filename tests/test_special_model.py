"""CPU side of the special-value and underflow tests: for every input the GPU tests launch (same generators, same seeds) the class
model of tests/special_model.py equals the classes of the oracle's result, the inputs meet the conditions the GPU tests assert
before a launch, and the oracle itself satisfies the derived bound for sums of subnormal products."""
import numpy as np
import pytest

import oracle
import special_model as sp
from util import value_class

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


@DTYPES
@pytest.mark.parametrize("name", sp.MATRICES)
def test_class_model_equals_the_oracle(name, dtype):
    n_rows, n_cols, off, col, val, share = sp.matrix(name, dtype)
    assert (np.abs(val) <= 1).all() and int(col.max()) < n_cols and len(off) == n_rows + 1
    lens = np.diff(off.astype(np.int64))
    for tag, v, x in sp.inputs(name, dtype):
        y = oracle.spmv(off, col, v, x)
        cls = sp.row_classes(off, col, v, x)
        assert np.array_equal(cls, value_class(y)), (name, tag)
        assert (cls[lens == 0] == 0).all() and not y[lens == 0].any()
        fin = sp.finite_share(off, cls)
        if tag == "x_sparse":
            assert 0.2 <= fin <= 0.8, (name, tag, fin)
        else:
            assert 0.0 < fin < 1.0, (name, tag, fin)
        if tag == "x_single":   # exactly the rows that reference the one column (NaN where a row holds it with both signs); no other NaN of x is read
            assert len(x) == n_cols + sp.X_TAIL and np.isnan(x[n_cols:]).all() and np.isinf(x).sum() == 1
            # where "every unreferenced column is NaN" bites: the matrices with columns nobody references (on the dense random ones
            # every column is referenced and only the NaN tail behind n_cols tests stray reads)
            unreferenced = int(np.isnan(x[:n_cols]).sum())
            assert unreferenced == n_cols - len(np.unique(col)) and unreferenced >= sp.UNREFERENCED_AT_LEAST.get(name, 0), (name, unreferenced)
            hit = np.zeros(n_rows, bool)
            hit[np.repeat(np.arange(n_rows), lens)[col == int(np.nonzero(np.isinf(x))[0][0])]] = True
            assert np.array_equal(cls != 0, hit) and hit.any()
            if lens.max() > 1000 and name != "tiled_skewed":
                assert (cls[lens > 1000] == 0).all()
        if tag.startswith("val_special"):
            bits = v.view(np.uint32 if dtype == np.float32 else np.uint64)
            for special in (np.inf, -np.inf, 0.0, -0.0):
                assert (bits == np.array([special], dtype).view(bits.dtype)[0]).any()
            assert np.isnan(v).any()
        if tag == "val_special+x_sparse":   # a stored zero meets an Inf somewhere: 0 * Inf = NaN
            with np.errstate(invalid="ignore"):
                assert ((v == 0) & np.isinf(x[col])).sum() >= 5, name


@DTYPES
@pytest.mark.parametrize("where", ["first", "last"])
def test_class_model_on_the_long_merge_row(dtype, where):
    off, col, val, x = sp.merge_long_row(dtype, where)
    cls = sp.row_classes(off, col, val, x)
    assert np.array_equal(cls, value_class(oracle.spmv(off, col, val, x)))
    assert cls[2] in (1, 2) and (np.delete(cls, 2) == 0).all() and np.isinf(val).sum() == 1


@DTYPES
@pytest.mark.parametrize("positive", [False, True], ids=["signed", "positive"])
@pytest.mark.parametrize("name", sp.UNDERFLOW_MATRICES)
def test_oracle_within_the_underflow_bound(name, dtype, positive):
    n_rows, n_cols, off, col, val, x = sp.underflow_inputs(name, dtype, positive)
    exact, bound = sp.underflow_bound(off, col, val, x)
    y = oracle.spmv(off, col, val, x)
    ratio = sp.underflow_ratio(y, exact, bound)
    print("underflow ratio oracle %s %s %s: %.3f" % (name, np.dtype(dtype).name, "positive" if positive else "signed", ratio))
    assert ratio <= 1.0
    tiny = np.finfo(dtype).tiny
    assert (np.abs(y[y != 0]) < tiny).any()                    # sums in the subnormal range ...
    if name == "ragged3001" and positive and dtype == np.float32:
        assert (np.abs(y) >= tiny).any()                       # ... and beyond it (f64: 2^13 entries would be needed; all adds are exact there)
    if positive:   # the bound discriminates: a result flushed to zero is outside it (all but rows whose only products are a few q themselves)
        flushed = np.abs(exact[bound > 0]) / bound[bound > 0]
        assert (flushed > 1.0).mean() > 0.99 and np.median(flushed) > 20, (flushed.min(), np.median(flushed))
