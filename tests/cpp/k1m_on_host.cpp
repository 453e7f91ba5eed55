// K1m's kernel source (sparsemat_amd/csrc/spmv_many.hip, copied next to this file's stand-in internal.hpp by
// tests/test_k1m_on_host.py) run on the CPU under AddressSanitizer / UBSan: every column bit for bit the storage-order sum, the
// padding columns +0 over NaN-prefilled storage and Inf in x's padding, nothing read or written outside exact-size arrays.
// argv[1] = "kt8": the KT = 8 body where ld allows it.
#include "spmv_many.inc"
#include <random>
template <typename T> static int run(int kind, size_t k, bool padded, bool kt8) {
    std::mt19937 rng(kind * 7 + k);
    const size_t n_rows = 700, n_cols = 901;
    std::vector<uint32_t> off(n_rows + 1, 0);
    for (size_t r = 0; r < n_rows; ++r) {
        uint32_t len = rng() % 10;
        if (kind == 1) len = 8;
        if (kind == 2) len = (rng() % 10 < 7) ? 0 : rng() % 4;
        if (kind == 3) { if (r >= 300 && r < 420) len = 60; if (r == 600) len = 5000; }
        if (kind == 4) len = rng() % 40;
        off[r + 1] = off[r] + len;
    }
    size_t nnz = off[n_rows];
    if (!padded && nnz % 4 == 0) { off[n_rows] += 1; nnz += 1; }
    // exact-size allocations: the sanitizer sees any read past what the kernel may touch
    const size_t alloc = padded ? nnz + 4 : nnz;
    uint32_t *col = new uint32_t[alloc]();
    T *val = new T[alloc]();
    std::uniform_real_distribution<double> u(-1, 1);
    for (size_t i = 0; i < nnz; ++i) { col[i] = rng() % n_cols; val[i] = (T)u(rng); }
    const size_t ld = (k + 3) & ~size_t(3);
    T *x = (T *)aligned_alloc(16, n_cols * ld * sizeof(T)), *y = (T *)aligned_alloc(16, n_rows * ld * sizeof(T));
    for (size_t i = 0; i < n_cols * ld; ++i) x[i] = (i % ld) < k ? (T)u(rng) : (T)INFINITY;  // garbage in the padding
    for (size_t i = 0; i < n_rows * ld; ++i) y[i] = (T)NAN;
    if (kt8) setenv("SMH_MANY_KT8", "1", 1);
    smh::launch_spmv_many(sizeof(T) == 8 ? SMH_F64 : SMH_F32, off.data(), col, val, x, y, n_rows, nnz, padded, k, ld, nullptr);
    int bad = 0;
    for (size_t r = 0; r < n_rows; ++r)
        for (size_t c = 0; c < ld; ++c) {
            T s = 0;
            if (c < k) for (uint32_t e = off[r]; e < off[r + 1]; ++e) { T p = x[(size_t)col[e] * ld + c] * val[e]; s = s + p; }
            if (std::memcmp(&s, &y[r * ld + c], sizeof(T)) != 0) ++bad;
        }
    delete[] col; delete[] val; free(x); free(y);
    std::printf("kind %d k %zu padded %d %s kt8 %d: %d wrong\n", kind, k, (int)padded, sizeof(T) == 8 ? "f64" : "f32", (int)kt8, bad);
    return bad;
}
int main(int argc, char **argv) {
    const bool kt8 = argc > 1;
    int bad = 0;
    bad += run<float>(3, 3, true, kt8);    // a tile beyond the stage, a row that straddles passes, padding columns
    bad += run<float>(4, 8, false, kt8);   // two groups (or one of eight), arrays that end inside a chunk
    bad += run<float>(2, 1, true, kt8);    // mostly empty rows
    bad += run<double>(3, 5, false, kt8);  // f64: a padded second group
    bad += run<double>(1, 8, true, kt8);   // f64, power-of-two rows
    std::printf("ok (%d failures)\n", bad);
    return bad != 0;
}
