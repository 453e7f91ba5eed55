// The multicolour ordering through the C++ mirror (include/sparsemat.hpp: color, then permute_symmetric and trisolve_levels) on the
// GPU.  argv[1]: a text file written by tests/test_cpp_color_gpu.py with any number of cases, each a square pattern and what the
// numpy model of the ordering (tests/color_model.py) expects for it -- n, nnz, seed, the offsets, the columns, the colours, the
// permutation, n_colors, n_rounds.
#include <cstdio>
#include <fstream>
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

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_color CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    size_t n_cases = 0;
    in >> n_cases;
    for (size_t k = 0; k < n_cases; ++k) {
        size_t n = 0, nnz = 0, n_colors = 0, n_rounds = 0;
        uint32_t seed = 0;
        in >> n >> nnz >> seed;
        std::vector<uint32_t> off(n + 1), col(nnz), want_colors(n), want_perm(n);
        for (auto &v : off) in >> v;
        for (auto &v : col) in >> v;
        for (auto &v : want_colors) in >> v;
        for (auto &v : want_perm) in >> v;
        in >> n_colors >> n_rounds;
        if (!in) { std::printf("cannot read case %zu of %s\n", k, argv[1]); return 2; }
        std::vector<double> val(nnz);
        for (size_t e = 0; e < nnz; ++e) val[e] = 1.0 + (double)e;
        auto a = SparseMatCRS<double>::from_raw_parts(n, n, off, col, val);

        SparseMatCRS<double>::ColorStats st;
        const std::vector<uint32_t> perm = a.color(seed, &st);
        CHECK(perm == want_perm);
        CHECK(st.colors == want_colors);
        CHECK(st.n_colors == n_colors && st.n_rounds == n_rounds);
        if (seed == 0) CHECK(a.color() == want_perm);  // (the default seed; the statistics are optional)

        // what it is for: the LOWER level of a row of the permuted matrix is its colour
        auto b = a.permute_symmetric(perm);
        const auto lower = b.trisolve_levels(SMH_TRI_LOWER), upper = b.trisolve_levels(SMH_TRI_UPPER);
        CHECK(lower.n_levels == n_colors && upper.n_levels <= n_colors);
        bool levels = lower.level_of_row.size() == n;
        for (size_t i = 0; i < n && levels; ++i) levels = lower.level_of_row[i] == want_colors[perm[i]];
        CHECK(levels);
    }
    auto rect = SparseMatCRS<double>::from_raw_parts(2, 3, {0, 1, 2}, {2, 0}, {1.0, 2.0});
    CHECK(panics([&] { rect.color(); }) == SMH_ERR_NOT_SQUARE);
    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
