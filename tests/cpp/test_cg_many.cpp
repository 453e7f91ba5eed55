// MultiVec<double>'s per-column BLAS-1 and ConjugateGradient::solve_many of the C++ mirror (include/sparsemat.hpp) on a small SPD
// system with k = 3 right-hand sides.  Built and run by tests/test_cpp_cg_many_gpu.py, which writes the case:
//   n nnz k | offsets | columns | value bits (hex) | k rows of b (hex bits) | tol iter_max | the model's k iteration counts
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
    size_t n = 0, nnz = 0, k = 0;
    in >> n >> nnz >> k;
    std::vector<uint32_t> off(n + 1), col(nnz);
    std::vector<double> val(nnz);
    for (auto &o : off) in >> o;
    for (auto &c : col) in >> c;
    std::string hex;
    for (auto &v : val) { in >> hex; v = from_hex(hex); }
    std::vector<std::vector<double>> b(k, std::vector<double>(n));
    for (auto &row : b)
        for (auto &v : row) { in >> hex; v = from_hex(hex); }
    double tol = 0.0;
    size_t iter_max = 0;
    in >> tol >> iter_max;
    std::vector<size_t> model_iters(k);
    for (auto &i : model_iters) in >> i;
    CHECK((bool)in && k == 3);

    auto m = SparseMatCRS<double>::from_raw_parts(n, n, off, col, val);
    MultiVec<double> B(b);

    // ---- the BLAS-1 members: against the same operations on the host, one rounding each
    {
        MultiVec<double> Z = B.copy();
        CHECK(Z.handle() != B.handle() && same_bits(Z.to_vecs()[1], b[1]));
        Z.add(B);
        Z.sub(B);
        Z.scale({2.0, -0.5, 3.0});
        const auto z = Z.to_vecs();
        const double f[3] = {2.0, -0.5, 3.0};
        for (size_t c = 0; c < 3; ++c) {
            std::vector<double> want(n);
            for (size_t i = 0; i < n; ++i) want[i] = ((b[c][i] + b[c][i]) - b[c][i]) * f[c];
            CHECK(same_bits(z[c], want));
        }
        const auto d = B.dot(Z), q = B.norm_squared();
        CHECK(d.size() == 3 && q.size() == 3);
        for (size_t c = 0; c < 3; ++c) {
            double s = 0.0, s2 = 0.0, mag = 0.0;
            for (size_t i = 0; i < n; ++i) { s += b[c][i] * z[c][i]; s2 += b[c][i] * b[c][i]; mag += std::fabs(b[c][i] * z[c][i]); }
            // two orders of summing n rounded terms differ by at most 2 n eps sum|t_i|
            CHECK(std::fabs(d[c] - s) <= 2.0 * n * 2.3e-16 * mag);
            CHECK(std::fabs(q[c] - s2) <= 2.0 * n * 2.3e-16 * s2);
        }
        int status = 0;
        try { Z.add(MultiVec<double>(n + 1, 3)); } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_DIM_MISMATCH);
        status = 0;
        try { Z.scale({1.0}); } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_DIM_MISMATCH);
    }

    // ---- solve_many: per-column counts and r.r as vectors
    MultiVec<double> X(n, 3);
    ConjugateGradient cg(tol, iter_max);
    cg.solve_many(m, B, X);
    CHECK(cg.iterations_many().size() == 3 && cg.r_norm_squared_many().size() == 3);
    const auto x = X.to_vecs();
    for (size_t c = 0; c < 3; ++c) {
        CHECK(cg.iterations_many()[c] == model_iters[c]);  // the model's count, exactly
        CHECK(std::sqrt(cg.r_norm_squared_many()[c]) < tol);
        // ConjugateGradient::solve of the column alone sums in another order: the same count within two bodies
        DenseVec<double> bc = DenseVec<double>::from_vec(b[c]), xc(n);
        ConjugateGradient one(tol, iter_max);
        one.solve(m, bc, xc);
        const long diff = (long)one.iterations() - (long)cg.iterations_many()[c];
        CHECK(diff >= -2 && diff <= 2);
        const auto x1 = xc.to_vec();
        double worst = 0.0;
        for (size_t i = 0; i < n; ++i) worst = std::fmax(worst, std::fabs(x1[i] - x[c][i]));
        CHECK(worst < 100.0 * tol);
    }
    // the residual b_c - A x_c of every column, without k downloads: the recursive residual is below tol, the true one differs
    // from it by rounding only (a few thousand eps here), far below 10 tol
    MultiVec<double> R = m.mvp_many(X);
    R.sub(B);
    for (double rr : R.norm_squared()) CHECK(std::sqrt(rr) < 10.0 * tol);

    // statuses through the mirror
    int status = 0;
    try { cg.solve_many(m, B, B); } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_INVALID);
    status = 0;
    try {
        MultiVec<double> X4(n, 4);
        cg.solve_many(m, B, X4);
    } catch (const Panic &p) { status = p.status; }
    CHECK(status == SMH_ERR_DIM_MISMATCH);
    CHECK(cg.iterations_many().size() == 3);  // (a refused call leaves the last results)

    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
