// The reordering operations through the C++ mirror (include/sparsemat.hpp: rcm, permute, permute_symmetric, bandwidth,
// DenseVec::permute) on the GPU.  argv[1]: a text file written by tests/test_cpp_reorder_gpu.py with a square pattern and what
// the numpy model of the ordering (tests/reorder_model.py) expects for it -- n, nnz, the offsets, the columns, the permutation,
// n_components, n_levels, the bandwidth of the reordered matrix.
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
    if (argc < 2) { std::printf("usage: test_reorder CASE\n"); return 2; }
    std::ifstream in(argv[1]);
    size_t n = 0, nnz = 0, comps = 0, levels = 0, band = 0;
    in >> n >> nnz;
    std::vector<uint32_t> off(n + 1), col(nnz), want(n);
    for (auto &v : off) in >> v;
    for (auto &v : col) in >> v;
    for (auto &v : want) in >> v;
    in >> comps >> levels >> band;
    if (!in) { std::printf("cannot read %s\n", argv[1]); return 2; }
    std::vector<double> val(nnz);
    for (size_t k = 0; k < nnz; ++k) val[k] = 1.0 + (double)k;
    auto a = SparseMatCRS<double>::from_raw_parts(n, n, off, col, val);

    SparseMatCRS<double>::RcmStats st;
    const std::vector<uint32_t> perm = a.rcm(&st);
    CHECK(perm == want);
    CHECK(st.n_components == comps && st.n_levels == levels);

    auto b = a.permute_symmetric(perm);
    CHECK(b.n_rows() == n && b.n_non_zero_entries() == nnz);
    const auto bw = b.bandwidth();
    CHECK(bw.first == band && bw.second == band);
    CHECK(a.bandwidth().first > band);
    // row i of b is row perm[i] of a, entry for entry, columns relabelled by the inverse
    std::vector<uint32_t> inv(n), boff, bcol;
    for (size_t i = 0; i < n; ++i) inv[perm[i]] = (uint32_t)i;
    std::vector<double> bval;
    b.raw_parts(boff, bcol, bval);
    bool same = true;
    for (size_t i = 0; i < n && same; ++i) {
        const uint32_t s0 = off[perm[i]], len = off[perm[i] + 1] - s0;
        same = boff[i + 1] - boff[i] == len;
        for (uint32_t k = 0; k < len && same; ++k) same = bcol[boff[i] + k] == inv[col[s0 + k]] && bval[boff[i] + k] == val[s0 + k];
    }
    CHECK(same);
    // permute(p, p) is the same matrix; the inverse brings a back
    std::vector<uint32_t> coff, ccol;
    std::vector<double> cval;
    a.permute(perm, perm).raw_parts(coff, ccol, cval);
    CHECK(coff == boff && ccol == bcol && cval == bval);
    b.permute(inv, inv).raw_parts(coff, ccol, cval);
    CHECK(coff == off && ccol == col && cval == val);
    a.permute({}, {}).raw_parts(coff, ccol, cval);
    CHECK(coff == off && ccol == col && cval == val);

    // solve-on-the-reordered-system bookkeeping: B x[p] = (A x)[p], and the scatter undoes the gather
    std::vector<double> x(n);
    for (size_t i = 0; i < n; ++i) x[i] = 0.25 * (double)(i % 17) - 1.0;
    const auto xv = DenseVec<double>::from_vec(x);
    const auto xp = xv.permute(perm);
    CHECK(xp.permute(perm, true).to_vec() == x);
    const std::vector<double> ya = a.mvp(xv, SMH_SPMV_SEQ).to_vec(), yb = b.mvp(xp, SMH_SPMV_SEQ).to_vec();
    bool prod = true;
    for (size_t i = 0; i < n; ++i) prod = prod && yb[i] == ya[perm[i]];
    CHECK(prod);

    // statuses arrive as Panics
    std::vector<uint32_t> bad = perm;
    bad[3] = bad[2];
    CHECK(panics([&] { a.permute_symmetric(bad); }) == SMH_ERR_INVALID);
    bad.pop_back();
    CHECK(panics([&] { a.permute_symmetric(bad); }) == SMH_ERR_DIM_MISMATCH);
    CHECK(panics([&] { xv.permute(bad); }) == SMH_ERR_DIM_MISMATCH);
    auto rect = SparseMatCRS<double>::from_raw_parts(2, 3, {0, 1, 2}, {2, 0}, {1.0, 2.0});
    CHECK(panics([&] { rect.rcm(); }) == SMH_ERR_NOT_SQUARE);
    CHECK(panics([&] { rect.permute_symmetric({1, 0}); }) == SMH_ERR_NOT_SQUARE);
    rect.permute({1, 0}, {2, 1, 0}).raw_parts(coff, ccol, cval);
    CHECK((ccol == std::vector<uint32_t>{2, 0}) && (cval == std::vector<double>{2.0, 1.0}));

    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
