// The non-symmetric FSAI and the solvers it preconditions through the C++ mirror (include/sparsemat.hpp) on a small non-symmetric
// convection-diffusion system: fsai_ns() and fsai_ns_apply(), GMRES::solve_fsai and BiCGStab::solve_fsai, both overloads, the pair
// passed and made by the solver.  Built and run by tests/test_cpp_pfsai_gpu.py, which writes the case:
//   n nnz | offsets | columns | value bits (hex) | b (hex bits) | tol iter_max restart
//   nnz of G_L | its values (hex bits) | nnz of G_U | its values (hex bits)
//   GMRES: the model's body count, cycle count and breakdown code | r.r (hex bits) | x (hex bits)
//   BiCGSTAB: the model's body count and breakdown code | r.r (hex bits) | x (hex bits)
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

static std::vector<double> read_hex(std::ifstream &in, size_t count) {
    std::vector<double> v(count);
    std::string hex;
    for (auto &x : v) { in >> hex; x = from_hex(hex); }
    return v;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: %s case.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    size_t n = 0, nnz = 0;
    in >> n >> nnz;
    std::vector<uint32_t> off(n + 1), col(nnz);
    for (auto &o : off) in >> o;
    for (auto &c : col) in >> c;
    const std::vector<double> val = read_hex(in, nnz), b = read_hex(in, n);
    double tol = 0.0;
    size_t iter_max = 0, restart = 0;
    in >> tol >> iter_max >> restart;
    size_t nnz_l = 0, nnz_u = 0;
    in >> nnz_l;
    const std::vector<double> model_gl = read_hex(in, nnz_l);
    in >> nnz_u;
    const std::vector<double> model_gu = read_hex(in, nnz_u);
    CHECK((bool)in && n > 0);

    auto m = SparseMatCRS<double>::from_raw_parts(n, n, off, col, val);

    // the factors: the model's bits; singular is optional
    size_t singular = 7;
    const auto f = m.fsai_ns(&singular);
    const SparseMatCRS<double> &gl = f.first, &gu = f.second;
    CHECK(singular == SparseMatCRS<double>::no_zero_pivot);
    CHECK(gl.n_rows() == n && gu.n_rows() == n && gl.n_non_zero_entries() == nnz_l && gu.n_non_zero_entries() == nnz_u);
    {
        std::vector<uint32_t> o, c;
        std::vector<double> v;
        gl.raw_parts(o, c, v);
        CHECK(same_bits(v, model_gl));
        gu.raw_parts(o, c, v);
        CHECK(same_bits(v, model_gu));
        const auto again = m.fsai_ns();
        again.second.raw_parts(o, c, v);
        CHECK(same_bits(v, model_gu));
    }
    // the application: two products, in place too, and smh_crs_fsai_apply_vec's bits
    {
        DenseVec<double> r = DenseVec<double>::from_vec(b), z(n), z2(n);
        gl.fsai_ns_apply(gu, r, z);
        gl.fsai_apply(gu, r, z2);
        CHECK(same_bits(z.to_vec(), z2.to_vec()) && same_bits(r.to_vec(), b));
        gl.fsai_ns_apply(gu, r, r);
        CHECK(same_bits(r.to_vec(), z.to_vec()));
    }

    // GMRES
    {
        size_t model_iters = 0, model_cycles = 0;
        int model_breakdown = -1;
        in >> model_iters >> model_cycles >> model_breakdown;
        const double model_rr = read_hex(in, 1)[0];
        const std::vector<double> model_x = read_hex(in, n);
        CHECK((bool)in);
        DenseVec<double> bd = DenseVec<double>::from_vec(b), xd(n);
        GMRES solver(tol, iter_max, restart);
        solver.solve_fsai(m, gl, gu, bd, xd);
        CHECK(solver.iterations() == model_iters && solver.cycles() == model_cycles && solver.breakdown() == model_breakdown);
        CHECK(solver.r_norm_squared() == model_rr && std::sqrt(solver.r_norm_squared()) < 2 * tol);
        CHECK(same_bits(xd.to_vec(), model_x) && same_bits(bd.to_vec(), b));
        std::vector<double> xh(n, 0.0), xo(n, 0.0);
        GMRES host(tol, iter_max, restart);
        host.solve_fsai(m, gl, gu, b, xh);
        CHECK(host.iterations() == model_iters && host.cycles() == model_cycles && same_bits(xh, model_x));
        host.solve_fsai(m, b, xo);  // ... factoring m itself
        CHECK(host.iterations() == model_iters && same_bits(xo, model_x));
        DenseVec<double> xd2(n);
        solver.solve_fsai(m, bd, xd2);
        CHECK(same_bits(xd2.to_vec(), model_x));
        int status = 0;
        try { solver.solve_fsai(m, gl, gu, bd, bd); } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_INVALID);
        status = 0;
        try {
            std::vector<double> short_x(n - 1, 0.0);
            host.solve_fsai(m, gl, gu, b, short_x);
        } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_DIM_MISMATCH);
        CHECK(solver.iterations() == model_iters);  // (a refused call leaves the last results)
    }

    // BiCGSTAB
    {
        size_t model_iters = 0;
        int model_breakdown = -1;
        in >> model_iters >> model_breakdown;
        const double model_rr = read_hex(in, 1)[0];
        const std::vector<double> model_x = read_hex(in, n);
        CHECK((bool)in);
        DenseVec<double> bd = DenseVec<double>::from_vec(b), xd(n);
        BiCGStab solver(tol, iter_max);
        solver.solve_fsai(m, gl, gu, bd, xd);
        CHECK(solver.iterations() == model_iters && solver.breakdown() == model_breakdown);
        CHECK(solver.r_norm_squared() == model_rr && std::sqrt(solver.r_norm_squared()) < tol);
        CHECK(same_bits(xd.to_vec(), model_x) && same_bits(bd.to_vec(), b));
        std::vector<double> xh(n, 0.0), xo(n, 0.0);
        BiCGStab host(tol, iter_max);
        host.solve_fsai(m, gl, gu, b, xh);
        CHECK(host.iterations() == model_iters && same_bits(xh, model_x));
        host.solve_fsai(m, b, xo);
        CHECK(host.iterations() == model_iters && same_bits(xo, model_x));
        int status = 0;
        try { solver.solve_fsai(m, gl, gu, bd, bd); } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_INVALID);
    }

    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
