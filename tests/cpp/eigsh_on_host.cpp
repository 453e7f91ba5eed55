// The host step of the eigensolver (sparsemat_amd/csrc/eigsh_host.hpp: eg_jacobi) as a program of its own, free of HIP.
// Built and run by tests/test_eigsh_on_host.py:  eigsh_on_host in.txt out.txt
//   in:  the number of matrices; per matrix m and its m x m entries (hex bits of f64, row-major)
//   out: per matrix the number of sweeps, theta (m hex words) and Y (m x m hex words, row-major)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "eigsh_host.hpp"

static double from_hex(const std::string &hex) {
    const unsigned long long b = std::strtoull(hex.c_str(), nullptr, 16);
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

static void put(std::FILE *f, const double *v, size_t count) {
    for (size_t i = 0; i < count; ++i) {
        unsigned long long b;
        std::memcpy(&b, v + i, sizeof b);
        std::fprintf(f, "%016llx%c", b, i + 1 == count ? '\n' : ' ');
    }
}

int main(int argc, char **argv) {
    if (argc < 3) { std::printf("usage: %s in.txt out.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::FILE *out = std::fopen(argv[2], "w");
    if (!out) return 2;
    size_t count = 0;
    in >> count;
    for (size_t c = 0; c < count; ++c) {
        int m = 0;
        in >> m;
        std::vector<double> b((size_t)m * m), y((size_t)m * m), theta(m);
        std::string hex;
        for (auto &v : b) { in >> hex; v = from_hex(hex); }
        if (!in) { std::printf("short input\n"); return 2; }
        const int sweeps = smh::eg_jacobi(m, b.data(), y.data(), theta.data());
        std::fprintf(out, "%d\n", sweeps);
        put(out, theta.data(), theta.size());
        put(out, y.data(), y.size());
    }
    std::fclose(out);
    std::printf("ok (%zu matrices)\n", count);
    return 0;
}
