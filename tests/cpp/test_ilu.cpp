// ilu0, ilu0_refactor, ilu_apply and ILUConjugateGradient of the C++ mirror (include/sparsemat.hpp) on a small five-point system in
// f64.  Built and run by tests/test_cpp_ilu_gpu.py, which writes the case:
//   n nnz | offsets | columns | value bits (hex) | b (hex bits) | tol iter_max | the model's body count | scale |
//   the model's factor | the model's factor of the scaled values | the model's U^-1 L^-1 b | the model's x   (hex bits each)
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
    size_t n = 0, nnz = 0;
    in >> n >> nnz;
    std::vector<uint32_t> off(n + 1), col(nnz);
    std::vector<double> val(nnz), b(n), model_f(nnz), model_f_scaled(nnz), model_z(n), model_x(n);
    for (auto &o : off) in >> o;
    for (auto &c : col) in >> c;
    std::string hex;
    for (auto &v : val) { in >> hex; v = from_hex(hex); }
    for (auto &v : b) { in >> hex; v = from_hex(hex); }
    double tol = 0.0, scale = 0.0;
    size_t iter_max = 0, model_iters = 0;
    in >> tol >> iter_max >> model_iters >> scale;
    for (auto *w : {&model_f, &model_f_scaled, &model_z, &model_x})
        for (auto &v : *w) { in >> hex; v = from_hex(hex); }
    CHECK((bool)in && n > 0);

    auto m = SparseMatCRS<double>::from_raw_parts(n, n, off, col, val);

    // the factor: an ordinary matrix on m's pattern
    size_t zero_pivot = 0;
    auto f = m.ilu0(&zero_pivot);
    CHECK(zero_pivot == SparseMatCRS<double>::no_zero_pivot);
    CHECK(f.n_rows() == n && f.n_non_zero_entries() == nnz);
    CHECK(same_bits(values_of(f), model_f));
    CHECK(same_bits(values_of(m), val));
    CHECK(f.trisolve_levels(SMH_TRI_LOWER).n_levels == m.trisolve_levels(SMH_TRI_LOWER).n_levels);

    // the application, out of place and in place
    DenseVec<double> bd = DenseVec<double>::from_vec(b), zd(n);
    f.ilu_apply(bd, zd);
    CHECK(same_bits(zd.to_vec(), model_z));
    CHECK(same_bits(bd.to_vec(), b));
    DenseVec<double> in_place = DenseVec<double>::from_vec(b);
    f.ilu_apply(in_place, in_place);
    CHECK(same_bits(in_place.to_vec(), model_z));

    // the solver: device and host vectors, a passed factor and its own
    DenseVec<double> xs(n);
    ILUConjugateGradient solver(tol, iter_max);
    solver.solve(m, f, bd, xs);
    CHECK(solver.iterations() == model_iters);
    CHECK(std::sqrt(solver.r_norm_squared()) < tol);
    CHECK(same_bits(xs.to_vec(), model_x));
    std::vector<double> xh(n, 0.0);
    ILUConjugateGradient host(tol, iter_max);
    host.solve(m, f, b, xh);
    CHECK(host.iterations() == model_iters && host.r_norm_squared() == solver.r_norm_squared());
    CHECK(same_bits(xh, model_x));
    std::vector<double> xo(n, 0.0);
    host.solve(m, b, xo);
    CHECK(same_bits(xo, model_x));

    // new values on the same pattern
    auto m2 = m.clone();
    m2.scale(scale);
    CHECK(f.ilu0_refactor(m2) == SparseMatCRS<double>::no_zero_pivot);
    CHECK(same_bits(values_of(f), model_f_scaled));
    CHECK(same_bits(values_of(m2.ilu0()), model_f_scaled));

    // statuses through the mirror
    int status = 0;
    try { solver.solve(m, f, bd, bd); } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_INVALID);
    status = 0;
    try {
        auto rect = SparseMatCRS<double>::from_raw_parts(1, 2, {0, 1}, {0}, {1.0});
        (void)rect.ilu0();
    } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_NOT_SQUARE);
    status = 0;
    try {
        auto unsorted = SparseMatCRS<double>::from_raw_parts(2, 2, {0, 2, 4}, {1, 0, 0, 1}, {1.0, 4.0, 1.0, 4.0});
        (void)unsorted.ilu0();
    } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_INVALID);
    status = 0;
    try {
        auto other = SparseMatCRS<double>::from_raw_parts(2, 2, {0, 1, 2}, {0, 1}, {1.0, 1.0});
        (void)f.ilu0_refactor(other);
    } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_DIM_MISMATCH);
    CHECK(same_bits(values_of(f), model_f_scaled));  // (a refused call leaves the factor)
    CHECK(solver.iterations() == model_iters);

    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
