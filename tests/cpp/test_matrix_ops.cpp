// Replays the reference's matrix addition / subtraction / scaling known answers (lostinc0de/sparsemat src/lib.rs:74-79,
// :104-107) through the operators of the C++ mirror (include/sparsemat.hpp: clone, add, sub, +=, -=, +, -, *=, * T) on the
// GPU, and the error cases as sparsemat::Panic.  Built and run by tests/test_cpp_matrix_ops_gpu.py.
#include <cstdio>
#include <string>
#include <vector>

#include "sparsemat.hpp"

using namespace sparsemat;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

template <typename F> static int panics(F f) {
    try {
        f();
    } catch (const Panic &p) {
        return p.status;
    }
    return 0;
}

int main() {
    // check_sparsemat_indexlist -> to_crs (src/lib.rs:54-82): the `sp` of the reference's test, as a CRS
    auto sp = SparseMatCRS<float>::from_raw_parts(3, 3, {0, 3, 5, 6}, {1, 2, 0, 2, 1, 2}, {4.2f, 0.12f, 7.12f, 4.12f, 2.24f, 2.12f});
    {
        auto sum = sp.clone() + sp.clone();
        CHECK(sum.get(0, 0) == 14.24f);                      // assert_eq!(sum.get(0, 0), 14.24)
        auto sub = sum.clone() - sp.clone();
        CHECK(sub.get(0, 0) == sp.get(0, 0));                // assert_eq!(sub.get(0, 0), sp.get(0, 0))
        auto mul = sp.clone() * 2.0f;
        CHECK(mul.get(0, 0) == sum.get(0, 0));               // assert_eq!(mul.get(0, 0), sum.get(0, 0))
        CHECK(sum.n_rows() == 3 && sum.n_cols() == 3 && sum.n_non_zero_entries() == 6);
    }
    {
        auto s = sp.clone();
        s += sp;                                             // sp.add(&sp_crs): row 1 reads "0 4.48 8.24 "
        CHECK(s.get(1, 0) == 0.0f && s.get(1, 1) == 4.48f && s.get(1, 2) == 8.24f);
        s -= sp;
        CHECK(s.get(1, 1) == 2.24f && s.get(1, 2) == 4.12f);
        s *= 2.0f;
        CHECK(s.get(1, 1) == 4.48f);
        s += s;                                              // aliasing: as if the right side had been cloned
        CHECK(s.get(1, 1) == 8.96f);
        s.sub(s);
        CHECK(s.get(1, 1) == 0.0f && s.n_non_zero_entries() == 6);  // exact zeros stay stored
    }
    {
        // a new entry is pushed to the START of its row; n_rows / n_cols grow only as far as new entries reach
        auto b = SparseMatCRS<float>::from_raw_parts(5, 9, {0, 1, 1, 1, 2, 2}, {0, 7}, {1.0f, -3.0f});
        auto c = sp + b;
        CHECK(c.n_rows() == 4 && c.n_cols() == 8 && c.n_non_zero_entries() == 7);
        std::vector<uint32_t> off, col;
        std::vector<float> val;
        c.raw_parts(off, col, val);
        CHECK(off[1] == 3 && col[2] == 0 && val[2] == 7.12f + 1.0f);  // (0,0) folded into the existing entry
        CHECK(off[4] == 7 && col[6] == 7 && val[6] == -3.0f);  // (3,7) opened row 3
        CHECK(sp.n_non_zero_entries() == 6);                    // + works on a clone
    }
    {
        // errors: Panic, the left operand unchanged
        auto d = SparseMatCRS<double>::from_raw_parts(3, 3, {0, 1, 2, 3}, {0, 1, 2}, {1.0, 2.0, 3.0});
        auto f = SparseMatCRS<float>::from_raw_parts(3, 3, {0, 1, 2, 3}, {0, 1, 2}, {1.0f, 2.0f, 3.0f});
        CHECK(panics([&] { d += SparseMatCRS<double>::from_raw_parts(0, 0, {0}, {}, {}); }) == 0);
        CHECK(panics([&] { smh_crs *out = nullptr; detail::check(smh_crs_add(d.handle(), f.handle(), &out)); }) == SMH_ERR_INVALID);
        CHECK(d.get(1, 1) == 2.0);
        SparseMatIndexList<float> one;
        one.add_to(3, 2, 1.0f);
        auto lone = one.as_direct_crs();                        // one push: no rows, one orphaned entry
        CHECK(lone.n_rows() == 0 && lone.orphans() == 1);
        CHECK(panics([&] { lone += f; }) == SMH_ERR_INVALID);
        CHECK(panics([&] { auto r = lone - f; (void)r; }) == SMH_ERR_INVALID);
        CHECK(lone.n_rows() == 0 && lone.orphans() == 1 && lone.n_cols() == 3);
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
