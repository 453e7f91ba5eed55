// fsai, fsai_apply and FSAIConjugateGradient of the C++ mirror (include/sparsemat.hpp) on a small five-point system in f64.  Built and
// run by tests/test_cpp_fsai_gpu.py, which writes the case:
//   n nnz nnz_g | offsets | columns | value bits (hex) | b (hex bits) | tol iter_max | the model's body count |
//   the model's G | the model's G^T | the model's G^T (G b) | the model's x   (hex bits each)
#include <cmath>
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

static double from_hex(const std::string &hex) {
    const unsigned long long b = std::strtoull(hex.c_str(), nullptr, 16);
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

static bool same_bits(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

static std::vector<double> values_of(const SparseMatCRS<double> &m) {
    std::vector<uint32_t> off, col;
    std::vector<double> val;
    m.raw_parts(off, col, val);
    return val;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: %s case.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    size_t n = 0, nnz = 0, nnz_g = 0;
    in >> n >> nnz >> nnz_g;
    std::vector<uint32_t> off(n + 1), col(nnz);
    std::vector<double> val(nnz), b(n), model_g(nnz_g), model_gt(nnz_g), model_z(n), model_x(n);
    for (auto &o : off) in >> o;
    for (auto &c : col) in >> c;
    std::string hex;
    for (auto &v : val) { in >> hex; v = from_hex(hex); }
    for (auto &v : b) { in >> hex; v = from_hex(hex); }
    double tol = 0.0;
    size_t iter_max = 0, model_iters = 0;
    in >> tol >> iter_max >> model_iters;
    for (auto *w : {&model_g, &model_gt, &model_z, &model_x})
        for (auto &v : *w) { in >> hex; v = from_hex(hex); }
    CHECK((bool)in && n > 0);

    auto m = SparseMatCRS<double>::from_raw_parts(n, n, off, col, val);

    // the pair: two ordinary matrices
    size_t not_spd = 0;
    auto f = m.fsai(&not_spd);
    const SparseMatCRS<double> &g = f.first, &gt = f.second;
    CHECK(not_spd == SparseMatCRS<double>::no_zero_pivot);
    CHECK(g.n_rows() == n && g.n_cols() == n && g.n_non_zero_entries() == nnz_g);
    CHECK(gt.n_rows() == n && gt.n_cols() == n && gt.n_non_zero_entries() == nnz_g);
    CHECK(same_bits(values_of(g), model_g));
    CHECK(same_bits(values_of(gt), model_gt));
    CHECK(same_bits(values_of(g.transpose()), model_gt));
    CHECK(same_bits(values_of(m), val));

    // the application, out of place and in place
    DenseVec<double> bd = DenseVec<double>::from_vec(b), zd(n);
    g.fsai_apply(gt, bd, zd);
    CHECK(same_bits(zd.to_vec(), model_z));
    CHECK(same_bits(bd.to_vec(), b));
    DenseVec<double> in_place = DenseVec<double>::from_vec(b);
    g.fsai_apply(gt, in_place, in_place);
    CHECK(same_bits(in_place.to_vec(), model_z));

    // the solver: device and host vectors, a passed pair and its own
    DenseVec<double> xs(n);
    FSAIConjugateGradient solver(tol, iter_max);
    solver.solve(m, g, gt, bd, xs);
    CHECK(solver.iterations() == model_iters);
    CHECK(std::sqrt(solver.r_norm_squared()) < tol);
    CHECK(same_bits(xs.to_vec(), model_x));
    std::vector<double> xh(n, 0.0);
    FSAIConjugateGradient host(tol, iter_max);
    host.solve(m, g, gt, b, xh);
    CHECK(host.iterations() == model_iters && host.r_norm_squared() == solver.r_norm_squared());
    CHECK(same_bits(xh, model_x));
    std::vector<double> xo(n, 0.0);
    host.solve(m, b, xo);
    CHECK(same_bits(xo, model_x));

    // statuses through the mirror
    int status = 0;
    try { solver.solve(m, g, gt, bd, bd); } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_INVALID);
    status = 0;
    try {
        auto rect = SparseMatCRS<double>::from_raw_parts(1, 2, {0, 1}, {0}, {1.0});
        (void)rect.fsai();
    } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_NOT_SQUARE);
    status = 0;
    try {
        auto unsorted = SparseMatCRS<double>::from_raw_parts(2, 2, {0, 2, 4}, {1, 0, 0, 1}, {1.0, 4.0, 1.0, 4.0});
        (void)unsorted.fsai();
    } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_INVALID);
    status = 0;
    auto other = SparseMatCRS<double>::from_raw_parts(2, 2, {0, 1, 2}, {0, 1}, {1.0, 1.0});
    try { solver.solve(m, other, gt, bd, xs); } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_DIM_MISMATCH);
    // not positive definite: reported by fsai(), a panic of the solver that factors by itself
    auto indefinite = SparseMatCRS<double>::from_raw_parts(2, 2, {0, 2, 4}, {0, 1, 0, 1}, {1.0, 2.0, 2.0, 1.0});
    (void)indefinite.fsai(&not_spd);
    CHECK(not_spd == 1);
    status = 0;
    std::vector<double> b2(2, 1.0), x2(2, 0.0);
    try { host.solve(indefinite, b2, x2); } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_INVALID && x2[0] == 0.0 && x2[1] == 0.0);
    CHECK(solver.iterations() == model_iters);

    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
