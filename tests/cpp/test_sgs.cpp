// The triangular solve, the SGS application and SGSConjugateGradient of the C++ mirror (include/sparsemat.hpp) on a small
// five-point system in f64.  Built and run by tests/test_cpp_sgs_gpu.py, which writes the case:
//   n nnz | offsets | columns | value bits (hex) | b (hex bits) | tol iter_max | the model's body count | levels lower upper |
//   the model's x | the model's lower solve of b | the model's upper unit solve of b | the model's M^-1 b   (hex bits each)
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

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: %s case.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    size_t n = 0, nnz = 0;
    in >> n >> nnz;
    std::vector<uint32_t> off(n + 1), col(nnz);
    std::vector<double> val(nnz), b(n), model_x(n), model_lower(n), model_upper_unit(n), model_z(n);
    for (auto &o : off) in >> o;
    for (auto &c : col) in >> c;
    std::string hex;
    for (auto &v : val) { in >> hex; v = from_hex(hex); }
    for (auto &v : b) { in >> hex; v = from_hex(hex); }
    double tol = 0.0;
    size_t iter_max = 0, model_iters = 0, levels_lower = 0, levels_upper = 0;
    in >> tol >> iter_max >> model_iters >> levels_lower >> levels_upper;
    for (auto *w : {&model_x, &model_lower, &model_upper_unit, &model_z})
        for (auto &v : *w) { in >> hex; v = from_hex(hex); }
    CHECK((bool)in && n > 0);

    auto m = SparseMatCRS<double>::from_raw_parts(n, n, off, col, val);

    // the level schedule and the solves
    const auto lo = m.trisolve_levels(SMH_TRI_LOWER), up = m.trisolve_levels(SMH_TRI_UPPER);
    CHECK(lo.n_levels == levels_lower && up.n_levels == levels_upper && lo.level_of_row.size() == n);
    CHECK(lo.n_launches == 1 && lo.small_level_rows >= 64 && lo.level_of_row[0] == 0);
    CHECK(same_bits(m.trisolve(b), model_lower));
    CHECK(same_bits(m.trisolve(b, SMH_TRI_UPPER, true), model_upper_unit));
    DenseVec<double> bd = DenseVec<double>::from_vec(b), xd(n);
    m.trisolve(bd, xd);
    CHECK(same_bits(xd.to_vec(), model_lower));
    m.trisolve(xd, xd, SMH_TRI_UPPER, true);  // in place
    DenseVec<double> zd(n);
    m.sgs_apply(bd, zd);
    CHECK(same_bits(zd.to_vec(), model_z));
    CHECK(same_bits(bd.to_vec(), b));

    // the solver, device and host vectors
    DenseVec<double> xs(n);
    SGSConjugateGradient solver(tol, iter_max);
    solver.solve(m, bd, xs);
    CHECK(solver.iterations() == model_iters);
    CHECK(std::sqrt(solver.r_norm_squared()) < tol);
    CHECK(same_bits(xs.to_vec(), model_x));
    std::vector<double> xh(n, 0.0);
    SGSConjugateGradient host(tol, iter_max);
    host.solve(m, b, xh);
    CHECK(host.iterations() == model_iters && host.r_norm_squared() == solver.r_norm_squared());
    CHECK(same_bits(xh, model_x));

    // statuses through the mirror
    int status = 0;
    try { solver.solve(m, bd, bd); } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_INVALID);
    status = 0;
    try {
        std::vector<double> short_b(n - 1, 0.0);
        (void)m.trisolve(short_b);
    } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_DIM_MISMATCH);
    status = 0;
    try { (void)m.trisolve(b, 7); } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_INVALID);
    CHECK(solver.iterations() == model_iters);  // (a refused call leaves the last results)

    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
