// Mixed precision through the C++ mirror (include/sparsemat.hpp) on the sorted convection-diffusion grid in f64: cast<U>() on
// SparseMatCRS and DenseVec, and IterativeRefinement with an ILU(0)-preconditioned GMRES(30) and an FSAI-preconditioned BiCGSTAB
// inside, both overloads, the f32 matrix and its factors passed and made by the solver.  Built and run by
// tests/test_cpp_refine_gpu.py, which writes the case:
//   n nnz | offsets | columns | value bits (hex) | the f32 values' bits (hex) | b (hex bits) | b in f32 (hex bits) | tol
//   per solve: the model's outer steps, inner bodies and code | r.r (hex bits) | x (hex bits)
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

template <typename T> static bool same_bits(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static std::vector<double> read_hex(std::ifstream &in, size_t count) {
    std::vector<double> v(count);
    std::string hex;
    for (auto &x : v) {
        in >> hex;
        const unsigned long long b = std::strtoull(hex.c_str(), nullptr, 16);
        std::memcpy(&x, &b, sizeof x);
    }
    return v;
}

static std::vector<float> read_hex32(std::ifstream &in, size_t count) {
    std::vector<float> v(count);
    std::string hex;
    for (auto &x : v) {
        in >> hex;
        const uint32_t b = (uint32_t)std::strtoul(hex.c_str(), nullptr, 16);
        std::memcpy(&x, &b, sizeof x);
    }
    return v;
}

struct Model {
    size_t outer = 0, iters = 0;
    int code = -1;
    double rr = 0.0;
    std::vector<double> x;
    void read(std::ifstream &in, size_t n) {
        in >> outer >> iters >> code;
        rr = read_hex(in, 1)[0];
        x = read_hex(in, n);
    }
};

static bool equals(const IterativeRefinement &s, const std::vector<double> &x, const Model &m) {
    return s.outer_iterations() == m.outer && s.iterations() == m.iters && s.code() == m.code && s.r_norm_squared() == m.rr && same_bits(x, m.x);
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: %s case.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    size_t n = 0, nnz = 0;
    in >> n >> nnz;
    std::vector<uint32_t> off(n + 1), col(nnz);
    for (auto &o : off) in >> o;
    for (auto &c : col) in >> c;
    const std::vector<double> val = read_hex(in, nnz);
    const std::vector<float> val32 = read_hex32(in, nnz);
    const std::vector<double> b = read_hex(in, n);
    const std::vector<float> b32 = read_hex32(in, n);
    double tol = 0.0;
    in >> tol;
    CHECK((bool)in && n > 0);

    auto m = SparseMatCRS<double>::from_raw_parts(n, n, off, col, val);

    // cast<U>(): numpy's bits, the pattern kept, exact on the way back, clone() on the same type
    size_t overflow = 7;
    const SparseMatCRS<float> lo = m.cast<float>(&overflow);
    {
        std::vector<uint32_t> o, c;
        std::vector<float> v;
        lo.raw_parts(o, c, v);
        CHECK(overflow == 0 && o == off && c == col && same_bits(v, val32));
        std::vector<double> w;
        lo.cast<double>().raw_parts(o, c, w);
        CHECK(w.size() == nnz);
        for (size_t k = 0; k < nnz && k < w.size(); ++k) CHECK(w[k] == (double)val32[k]);
        m.cast<double>().raw_parts(o, c, w);
        CHECK(same_bits(w, val));
        const DenseVec<double> bd = DenseVec<double>::from_vec(b);
        const DenseVec<float> down = bd.cast<float>();
        CHECK(same_bits(down.to_vec(), b32) && same_bits(bd.cast<double>().to_vec(), b));
        CHECK(down.cast<double>().to_vec()[0] == (double)b32[0]);
    }

    Model gmres, bicgstab;
    gmres.read(in, n);
    bicgstab.read(in, n);
    CHECK((bool)in);

    // GMRES(30) with ILU(0) inside
    {
        const SparseMatCRS<float> f = lo.ilu0();
        DenseVec<double> bd = DenseVec<double>::from_vec(b), xd(n);
        IterativeRefinement solver(tol, 20, SMH_INNER_GMRES, SMH_PRECOND_ILU);
        solver.solve(m, lo, &f, nullptr, bd, xd);
        CHECK(equals(solver, xd.to_vec(), gmres) && same_bits(bd.to_vec(), b));
        CHECK(solver.code() == 0 && std::sqrt(solver.r_norm_squared()) < tol);
        std::vector<double> xh(n, 0.0), xo(n, 0.0), xc(n, 0.0);
        solver.solve(m, lo, &f, nullptr, b, xh);
        CHECK(equals(solver, xh, gmres));
        solver.solve(m, lo, b, xo);  // ... factoring lo itself
        CHECK(equals(solver, xo, gmres));
        solver.solve(m, b, xc);      // ... casting m itself
        CHECK(equals(solver, xc, gmres));
        DenseVec<double> xd2(n);
        solver.solve(m, bd, xd2);
        CHECK(equals(solver, xd2.to_vec(), gmres));
        int status = 0;
        try { solver.solve(m, lo, &f, nullptr, bd, bd); } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_INVALID);
        status = 0;
        try { solver.solve(m, lo, nullptr, nullptr, bd, xd2); } catch (const Panic &p) { status = p.status; }  // (ILU takes a factor)
        CHECK(status == SMH_ERR_INVALID);
        status = 0;
        try {
            std::vector<double> short_x(n - 1, 0.0);
            solver.solve(m, lo, &f, nullptr, b, short_x);
        } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_DIM_MISMATCH);
        CHECK(solver.iterations() == gmres.iters);  // (a refused call leaves the last results)
    }

    // BiCGSTAB with the non-symmetric FSAI inside
    {
        const auto f = lo.fsai_ns();
        DenseVec<double> bd = DenseVec<double>::from_vec(b), xd(n);
        IterativeRefinement solver(tol, 20, SMH_INNER_BICGSTAB, SMH_PRECOND_FSAI);
        solver.solve(m, lo, &f.first, &f.second, bd, xd);
        CHECK(equals(solver, xd.to_vec(), bicgstab));
        std::vector<double> xo(n, 0.0);
        solver.solve(m, b, xo);
        CHECK(equals(solver, xo, bicgstab));
        int status = 0;
        try { IterativeRefinement(tol, 20, SMH_INNER_CG, SMH_PRECOND_JACOBI).solve(m, b, xo); } catch (const Panic &p) { status = p.status; }
        CHECK(status == SMH_ERR_INVALID);
    }

    std::printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
