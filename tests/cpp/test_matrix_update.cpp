// Replays the reference's SparseMatCRS test (lostinc0de/sparsemat src/lib.rs:114-154) through SparseMatCRS::add_to of the C++
// mirror (include/sparsemat.hpp), one device call per add_to starting from SparseMatCRS::new(), and checks eye, get and a
// batched apply.  Built and run by tests/test_cpp_update_gpu.py.
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

int main() {
    {  // check_sparsemat_crs (src/lib.rs:114-154)
        auto sp = SparseMatCRS<float>::new_empty();
        sp.add_to(0, 1, 4.2f);
        sp.add_to(2, 2, 2.12f);
        sp.add_to(1, 2, 4.12f);
        sp.add_to(3, 2, 1.12f);
        sp.add_to(3, 3, 5.12f);
        std::vector<uint32_t> off, col;
        std::vector<float> val;
        sp.raw_parts(off, col, val);
        CHECK((off == std::vector<uint32_t>{0, 1, 2, 3, 5}));
        CHECK((col == std::vector<uint32_t>{1, 2, 2, 3, 2}));  // the iteration order of the reference's iter()
        CHECK((val == std::vector<float>{4.2f, 4.12f, 2.12f, 5.12f, 1.12f}));
        CHECK(sp.orphans() == 0);
        std::vector<uint32_t> rows, col_ptr, entries;
        sp.column_info(rows, col_ptr, entries);
        std::vector<float> c2;
        for (uint32_t e = col_ptr[2]; e < col_ptr[3]; ++e) c2.push_back(val[entries[e]]);
        CHECK((c2 == std::vector<float>{4.12f, 2.12f, 1.12f}));  // iter_col(2)
        CHECK(sp.get(0, 1) == 4.2f && sp.get(5, 0) == 0.0f && sp.get(3, 2) == 1.12f && sp.get(0, 0) == 0.0f);
        auto v = DenseVec<float>::from_vec({2.0f, 4.8f, 1.2f, 3.4f});
        auto y = sp * v;
        CHECK(y.get(0) == 20.16f);                     // assert_eq!(mvp.get(0), 20.16)
        CHECK(sp.density() == 5.0 / 16.0);             // assert_eq!(sp_crs.density(), 5.0 / 16.0)
        // a batched stream: re-assembly into the same pattern plus one set
        sp.apply({3, 0, 3}, {2, 1, 2}, {1.0f, 0.5f, 7.0f}, {0, 0, 1});
        CHECK(sp.get(3, 2) == 7.0f && sp.get(0, 1) == 4.7f);
        auto g = sp.get_many({3, 0, 9}, {3, 1, 0});
        CHECK((g == std::vector<float>{5.12f, 4.7f, 0.0f}));
        int status = 0;
        try {
            sp.add_to((size_t(1) << 32) + 1, 0, 1.0f);  // beyond Index = u32: refused, not truncated to row 1
        } catch (const Panic &p) {
            status = p.status;
        }
        CHECK(status == SMH_ERR_INVALID);
        CHECK(sp.get(1, 0) == 0.0f && sp.n_non_zero_entries() == 5);
    }
    {  // eye(3) * v == v
        auto e = SparseMatCRS<double>::eye(3);
        CHECK(e.n_rows() == 3 && e.n_cols() == 3 && e.n_non_zero_entries() == 3);
        auto v = DenseVec<double>::from_vec({1.5, -2.25, 3.0});
        auto y = e * v;
        CHECK(y.get(0) == 1.5 && y.get(1) == -2.25 && y.get(2) == 3.0);
        CHECK(e.get(1, 1) == 1.0 && e.get(1, 2) == 0.0);
        auto e1 = SparseMatCRS<double>::eye(1);  // the first push alone: no rows, one orphan
        CHECK(e1.n_rows() == 0 && e1.n_cols() == 1 && e1.orphans() == 1);
    }
    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
