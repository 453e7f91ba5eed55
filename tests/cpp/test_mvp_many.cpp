// The reference's two known-answer matrices (lostinc0de/sparsemat src/lib.rs:54-98 and :114-154; tests/golden/reference_kats.json)
// through MultiVec<float> and SparseMatCRS<float>::mvp_many of the C++ mirror (include/sparsemat.hpp), k = 3 columns, the middle
// one the reference's vector: its row 0 is the reference's 34.544 / 20.16, every column equals the single product bit for bit.
// Built and run by tests/test_cpp_mvp_many_gpu.py, which writes the cases from the golden file:
//   n_rows n_cols nnz | offsets | columns | value bits (hex) | x (decimal literals) | expected mvp.get(0) (decimal literal)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sparsemat.hpp"

using namespace sparsemat;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: %s cases.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    size_t n_cases = 0;
    in >> n_cases;
    CHECK(n_cases == 2);
    for (size_t q = 0; q < n_cases; ++q) {
        size_t n_rows = 0, n_cols = 0, nnz = 0;
        in >> n_rows >> n_cols >> nnz;
        std::vector<uint32_t> off(n_rows + 1), col(nnz);
        std::vector<float> val(nnz), x(n_cols);
        for (auto &o : off) in >> o;
        for (auto &c : col) in >> c;
        for (auto &v : val) {
            std::string hex;
            in >> hex;
            const uint32_t b = (uint32_t)std::strtoul(hex.c_str(), nullptr, 16);
            std::memcpy(&v, &b, sizeof v);
        }
        std::string lit;
        for (auto &e : x) { in >> lit; e = std::strtof(lit.c_str(), nullptr); }
        in >> lit;
        const float expect0 = std::strtof(lit.c_str(), nullptr);
        CHECK((bool)in);

        auto m = SparseMatCRS<float>::from_raw_parts(n_rows, n_cols, off, col, val);
        std::vector<std::vector<float>> cols3(3, std::vector<float>(n_cols));
        for (size_t i = 0; i < n_cols; ++i) {
            cols3[0][i] = 0.5f - (float)i;   // a column before ...
            cols3[1][i] = x[i];              // ... the reference's vector ...
            cols3[2][i] = 1.0f / (float)(i + 3);  // ... and one behind it
        }
        MultiVec<float> X(cols3);
        CHECK(X.dim() == n_cols && X.count() == 3 && smh_mvec_ld(X.handle()) == 4);
        CHECK(X.to_vecs() == cols3);
        MultiVec<float> Y = m.mvp_many(X);
        CHECK(Y.dim() == n_rows && Y.count() == 3);
        const auto y = Y.to_vecs();
        CHECK(y[1][0] == expect0);  // assert_eq!(mvp.get(0), 34.544) / (…, 20.16)
        for (size_t c = 0; c < 3; ++c) {
            CHECK(same_bits(y[c], m.mvp(cols3[c], SMH_SPMV_SEQ)));
            CHECK(same_bits(Y.column(c).to_vec(), y[c]));
            CHECK(same_bits(X.column(c).to_vec(), cols3[c]));
        }
        // set_column: the product follows the new column, its neighbours stay
        X.set_column(2, DenseVec<float>::from_vec(x));
        const auto y2 = m.mvp_many(X).to_vecs();
        CHECK(same_bits(y2[2], y[1]) && same_bits(y2[0], y[0]) && same_bits(y2[1], y[1]));
        // statuses through the mirror: a column beyond k, a vector of another dimension, x beyond the columns' reach
        int status = 0;
        try { X.column(3); } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_INVALID);
        status = 0;
        try { X.set_column(0, DenseVec<float>(n_cols + 1)); } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_DIM_MISMATCH);
        status = 0;
        try { m.mvp_many(MultiVec<float>(n_cols - 1, 3)); } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_INDEX_RANGE);
        // moved-from: inert
        MultiVec<float> Z = std::move(Y);
        CHECK(Y.handle() == nullptr && Z.count() == 3);
    }
    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
