// Lanczos of the C++ mirror (include/sparsemat.hpp) on a small symmetric tridiagonal matrix, every overload.
// Built and run by tests/test_cpp_eigsh_gpu.py, which writes the case:
//   n nnz | offsets | columns | value bits (hex) | start (hex bits) | k ncv which tol restart_max | the model's n_conv, restarts,
//   products and breakdown code | the model's values (hex bits) | its estimates | its vectors, k x n
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
    std::vector<double> val(nnz), start(n);
    for (auto &o : off) in >> o;
    for (auto &c : col) in >> c;
    std::string hex;
    for (auto &v : val) { in >> hex; v = from_hex(hex); }
    for (auto &v : start) { in >> hex; v = from_hex(hex); }
    size_t k = 0, ncv = 0, restart_max = 0, model_n_conv = 0, model_restarts = 0, model_products = 0;
    int which = -1, model_breakdown = -1;
    double tol = 0.0;
    in >> k >> ncv >> which >> tol >> restart_max >> model_n_conv >> model_restarts >> model_products >> model_breakdown;
    std::vector<double> model_values(k), model_est(k);
    std::vector<std::vector<double>> model_vectors(k, std::vector<double>(n));
    for (auto &v : model_values) { in >> hex; v = from_hex(hex); }
    for (auto &v : model_est) { in >> hex; v = from_hex(hex); }
    for (auto &x : model_vectors)
        for (auto &v : x) { in >> hex; v = from_hex(hex); }
    CHECK((bool)in && n > 0 && k > 0);

    auto m = SparseMatCRS<double>::from_raw_parts(n, n, off, col, val);

    // device vectors
    DenseVec<double> sd = DenseVec<double>::from_vec(start);
    MultiVec<double> xd(n, k);
    Lanczos solver(k, which, tol, ncv, restart_max);
    solver.solve(m, sd, xd);
    CHECK(solver.n_conv() == model_n_conv && solver.n_conv() == k);  // the model's counts, exactly: a converged case
    CHECK(solver.restarts() == model_restarts && solver.products() == model_products && solver.breakdown() == model_breakdown);
    CHECK(same_bits(solver.values(), model_values) && same_bits(solver.estimates(), model_est));
    const auto got = xd.to_vecs();
    for (size_t c = 0; c < k; ++c) CHECK(same_bits(got[c], model_vectors[c]));
    CHECK(same_bits(sd.to_vec(), start));

    // no vectors: the same values
    Lanczos plain(k, which, tol, ncv, restart_max);
    plain.solve(m, sd);
    CHECK(same_bits(plain.values(), model_values) && plain.products() == model_products);

    // host vectors: the same solve
    std::vector<std::vector<double>> xh;
    Lanczos host(k, which, tol, ncv, restart_max);
    host.solve(m, start, xh);
    CHECK(host.n_conv() == model_n_conv && host.restarts() == model_restarts && host.products() == model_products && host.breakdown() == model_breakdown);
    CHECK(same_bits(host.values(), model_values) && same_bits(host.estimates(), model_est) && xh.size() == k);
    for (size_t c = 0; c < k && c < xh.size(); ++c) CHECK(same_bits(xh[c], model_vectors[c]));

    // a breakdown is a result, not a panic: a zero start is code 2, nothing returned, no product
    std::vector<double> zero(n, 0.0);
    std::vector<std::vector<double>> none;
    Lanczos broken(k, which, tol, ncv, restart_max);
    broken.solve(m, zero, none);
    CHECK(broken.breakdown() == 2 && broken.products() == 0 && broken.n_conv() == 0 && broken.values().empty() && none.empty());

    // statuses through the mirror
    int status = 0;
    try {
        MultiVec<double> wrong(n, k + 1);
        solver.solve(m, sd, wrong);
    } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_INVALID);
    status = 0;
    try {
        std::vector<double> short_start(n - 1, 1.0);
        host.solve(m, short_start, xh);
    } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_DIM_MISMATCH);
    status = 0;
    try {
        Lanczos narrow(k, which, tol, k + 1, restart_max);
        narrow.solve(m, sd);
    } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_INVALID);

    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
