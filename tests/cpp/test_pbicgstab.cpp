// The preconditioner option of the C++ mirror's BiCGStab (include/sparsemat.hpp) on a small non-symmetric convection-diffusion
// system: Jacobi, SGS and ILU(0), both overloads, the factor passed and made by the solver.  Built and run by
// tests/test_cpp_pbicgstab_gpu.py, which writes the case:
//   n nnz | offsets | columns | value bits (hex) | b (hex bits) | tol iter_max | then per kind (SMH_PRECOND_JACOBI, _SGS, _ILU):
//   the model's body count and breakdown code | the model's r.r (hex bits) | the model's x (hex bits)
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
    std::vector<double> val(nnz), b(n);
    for (auto &o : off) in >> o;
    for (auto &c : col) in >> c;
    std::string hex;
    for (auto &v : val) { in >> hex; v = from_hex(hex); }
    for (auto &v : b) { in >> hex; v = from_hex(hex); }
    double tol = 0.0;
    size_t iter_max = 0;
    in >> tol >> iter_max;
    CHECK((bool)in && n > 0);

    auto m = SparseMatCRS<double>::from_raw_parts(n, n, off, col, val);
    const SparseMatCRS<double> factor = m.ilu0();

    const int kinds[3] = {SMH_PRECOND_JACOBI, SMH_PRECOND_SGS, SMH_PRECOND_ILU};
    for (int kind : kinds) {
        size_t model_iters = 0;
        int model_breakdown = -1;
        std::vector<double> model_x(n);
        in >> model_iters >> model_breakdown;
        in >> hex;
        const double model_rr = from_hex(hex);
        for (auto &v : model_x) { in >> hex; v = from_hex(hex); }
        CHECK((bool)in);

        // device vectors (ILU: the solver factors mat itself)
        DenseVec<double> bd = DenseVec<double>::from_vec(b), xd(n);
        BiCGStab solver(tol, iter_max, kind);
        solver.solve(m, bd, xd);
        CHECK(solver.iterations() == model_iters);  // the model's count, exactly
        CHECK(solver.breakdown() == model_breakdown);
        CHECK(solver.r_norm_squared() == model_rr && std::sqrt(solver.r_norm_squared()) < 2 * tol);
        CHECK(same_bits(xd.to_vec(), model_x));
        CHECK(same_bits(bd.to_vec(), b));

        // host vectors: the same solve
        std::vector<double> xh(n, 0.0);
        BiCGStab host(tol, iter_max, kind);
        host.solve(m, b, xh);
        CHECK(host.iterations() == model_iters && host.breakdown() == model_breakdown);
        CHECK(host.r_norm_squared() == solver.r_norm_squared());
        CHECK(same_bits(xh, model_x));

        // a factor goes with SMH_PRECOND_ILU alone: the same bits there, the library's refusal elsewhere
        std::vector<double> xf(n, 0.0);
        int status = 0;
        try { host.solve(m, factor, b, xf); } catch (const Panic &p) { status = p.status; }
        if (kind == SMH_PRECOND_ILU) CHECK(status == 0 && same_bits(xf, model_x));
        else CHECK(status == SMH_ERR_INVALID && same_bits(xf, std::vector<double>(n, 0.0)));

        // statuses through the mirror
        status = 0;
        try { solver.solve(m, bd, bd); } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_INVALID);
        status = 0;
        try {
            std::vector<double> short_x(n - 1, 0.0);
            solver.solve(m, b, short_x);
        } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_DIM_MISMATCH);
        CHECK(solver.iterations() == model_iters);  // (a refused call leaves the last results)
    }

    // the default is the unpreconditioned solver
    std::vector<double> xp(n, 0.0), xn(n, 0.0);
    BiCGStab plain(tol, iter_max), none(tol, iter_max, SMH_PRECOND_NONE);
    plain.solve(m, b, xp);
    none.solve(m, b, xn);
    CHECK(same_bits(xp, xn) && plain.iterations() == none.iterations() && plain.r_norm_squared() == none.r_norm_squared());

    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
