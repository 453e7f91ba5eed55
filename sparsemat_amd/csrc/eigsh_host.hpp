// eigsh_host.hpp -- the host step of the thick-restart Lanczos eigensolver (eigsh.hip): plain C++ in f64, free of HIP, so that a
// stand-alone host program (tests/cpp/eigsh_on_host.cpp) exercises it and tests/eigsh_model.py restates it operation for operation.
// Only + - * / sqrt and comparisons; the build passes -ffp-contract=off, so nothing is contracted.
//
// eg_jacobi(m, B, Y, theta): the cyclic Jacobi diagonalisation of the symmetric m x m matrix B (row-major, both triangles stored and
// kept equal), the rotations accumulated into Y (row-major, Y = I at the start): B = Y diag(theta) Y^T.
//   sweep order:  p = 0 .. m-2, q = p+1 .. m-1 (row-cyclic)
//   skip rule:    a = B[p][q];  when |B[p][p]| + |a| == |B[p][p]| and |B[q][q]| + |a| == |B[q][q]| (a == 0 is one such case) the pair
//                 is skipped and B[p][q] = B[q][p] = 0 (no rotation is counted)
//   rotation:     tau = (B[q][q] - B[p][p]) / (2 a);  t = 1 / (|tau| + sqrt(1 + tau tau)), negated when tau < 0;
//                 c = 1 / sqrt(1 + t t);  s = t c;  h = t a
//                 for every r:  (x, y) = (B[r][p], B[r][q]);  B[r][p] = B[p][r] = c x - s y;  B[r][q] = B[q][r] = s x + c y
//                 then  B[p][p] = (old B[p][p]) - h;  B[q][q] = (old B[q][q]) + h;  B[p][q] = B[q][p] = 0
//                 for every r:  (x, y) = (Y[r][p], Y[r][q]);  Y[r][p] = c x - s y;  Y[r][q] = s x + c y
//                 (tau tau may overflow to +inf for a tiny a: t = 0, c = 1, s = 0 and the pair is zeroed: still finite)
//   stop rule:    after a sweep in which no rotation was made, or after kEgMaxSweeps sweeps (so it terminates on any finite input;
//                 non-finite input never reaches it: breakdown 3)
//   theta:        the diagonal, sorted ascending by a stable insertion sort (ties by index); Y's columns are permuted with it
// eg_cycle_end<T>: a cycle's decisions (the recurrence is in eigsh.hip's header).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace smh {

constexpr int kEgMaxM = 128;
constexpr int kEgMaxSweeps = 64;

inline double eg_abs(double x) { return x < 0 ? -x : x; }
inline bool eg_finite(double x) { return x - x == 0; }  // (false for NaN and +-inf)

// returns the number of sweeps made (the last one found nothing to rotate, unless the cap was hit)
inline int eg_jacobi(int m, double *B, double *Y, double *theta) {
    for (int i = 0; i < m; ++i)
        for (int c = 0; c < m; ++c) Y[(size_t)i * m + c] = i == c ? 1.0 : 0.0;
    int sweeps = 0;
    while (sweeps < kEgMaxSweeps) {
        ++sweeps;
        int rotations = 0;
        for (int p = 0; p + 1 < m; ++p) {
            for (int q = p + 1; q < m; ++q) {
                const double a = B[(size_t)p * m + q], bpp = B[(size_t)p * m + p], bqq = B[(size_t)q * m + q];
                const double abs_a = eg_abs(a), abs_p = eg_abs(bpp), abs_q = eg_abs(bqq);
                if (abs_p + abs_a == abs_p && abs_q + abs_a == abs_q) {
                    B[(size_t)p * m + q] = B[(size_t)q * m + p] = 0.0;
                    continue;
                }
                ++rotations;
                const double tau = (bqq - bpp) / (2.0 * a);
                double t = 1.0 / (eg_abs(tau) + std::sqrt(1.0 + tau * tau));
                if (tau < 0) t = -t;
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c, h = t * a;
                for (int r = 0; r < m; ++r) {
                    const double x = B[(size_t)r * m + p], y = B[(size_t)r * m + q];
                    const double np = c * x - s * y, nq = s * x + c * y;
                    B[(size_t)r * m + p] = B[(size_t)p * m + r] = np;
                    B[(size_t)r * m + q] = B[(size_t)q * m + r] = nq;
                }
                B[(size_t)p * m + p] = bpp - h;
                B[(size_t)q * m + q] = bqq + h;
                B[(size_t)p * m + q] = B[(size_t)q * m + p] = 0.0;
                for (int r = 0; r < m; ++r) {
                    const double x = Y[(size_t)r * m + p], y = Y[(size_t)r * m + q];
                    Y[(size_t)r * m + p] = c * x - s * y;
                    Y[(size_t)r * m + q] = s * x + c * y;
                }
            }
        }
        if (rotations == 0) break;
    }
    // ascending, ties by index: a stable insertion sort of the indices
    std::vector<int> order(m);
    for (int i = 0; i < m; ++i) {
        int at = i;
        while (at > 0 && B[(size_t)order[at - 1] * m + order[at - 1]] > B[(size_t)i * m + i]) {
            order[at] = order[at - 1];
            --at;
        }
        order[at] = i;
    }
    std::vector<double> ys((size_t)m * m);
    for (int i = 0; i < m; ++i) {
        theta[i] = B[(size_t)order[i] * m + order[i]];
        for (int r = 0; r < m; ++r) ys[(size_t)r * m + i] = Y[(size_t)r * m + order[i]];
    }
    for (size_t i = 0; i < (size_t)m * m; ++i) Y[i] = ys[i];
    return sweeps;
}

// What the host keeps of a solve between its cycles, and the workspaces of the host step (allocated once, before the first cycle).
template <typename T>
struct EgHost {
    int k = 0, m = 0, which = 0;
    double tol = 0.0;
    int l = 0;                   // locked Ritz vectors the cycle began with
    T theta_l[kEgMaxM], s_l[kEgMaxM];  // their Ritz values and couplings, in T
    std::vector<double> B, Y, theta, est;  // m x m, m x m, m, m (est in the wanted order)
    std::vector<int> wanted;               // Ritz pair indices, wanted-first
    int n_conv = 0;
    void init(int k_, int m_, int which_, double tol_) {
        k = k_; m = m_; which = which_; tol = tol_; l = 0; n_conv = 0;
        B.assign((size_t)m * m, 0.0); Y.assign((size_t)m * m, 0.0); theta.assign(m, 0.0); est.assign(m, 0.0); wanted.assign(m, 0);
    }
};

// The cycle end after mc columns (mc = m, or fewer after breakdown 1); alpha, beta: indexed by column, entries l .. mc-1 valid.
// Returns false when a value is not finite (breakdown 3: nothing else is done).  Else theta (ascending), Y, wanted, est and n_conv
// (the converged prefix of the wanted order, at most min(k, mc) long) are set.
template <typename T>
bool eg_cycle_end(EgHost<T> &h, int mc, const T *alpha, const T *beta) {
    const int l = h.l;
    for (int i = 0; i < l; ++i)
        if (!eg_finite((double)h.theta_l[i]) || !eg_finite((double)h.s_l[i])) return false;
    for (int j = l; j < mc; ++j)
        if (!eg_finite((double)alpha[j]) || !eg_finite((double)beta[j])) return false;
    double *B = h.B.data();
    for (size_t i = 0; i < (size_t)mc * mc; ++i) B[i] = 0.0;
    for (int i = 0; i < l; ++i) {
        B[(size_t)i * mc + i] = (double)h.theta_l[i];
        B[(size_t)i * mc + l] = B[(size_t)l * mc + i] = (double)h.s_l[i];
    }
    for (int j = l; j < mc; ++j) {
        B[(size_t)j * mc + j] = (double)alpha[j];
        if (j + 1 < mc) B[(size_t)j * mc + j + 1] = B[(size_t)(j + 1) * mc + j] = (double)beta[j];
    }
    eg_jacobi(mc, B, h.Y.data(), h.theta.data());
    double thmax = 0.0;
    for (int i = 0; i < mc; ++i) {
        h.wanted[i] = h.which == 0 ? mc - 1 - i : i;
        const double a = eg_abs(h.theta[i]);
        if (a > thmax) thmax = a;
    }
    const double bl = (double)beta[mc - 1];
    for (int i = 0; i < mc; ++i) h.est[i] = eg_abs(bl * h.Y[(size_t)(mc - 1) * mc + h.wanted[i]]);
    const int kk = h.k < mc ? h.k : mc;
    h.n_conv = 0;
    while (h.n_conv < kk && h.est[h.n_conv] <= h.tol * thmax) ++h.n_conv;
    return true;
}

// Yt (mc rows of ldy values, zero beyond `cols`) = T(Y[:, the first `cols` wanted]); lock: the restart's theta_i = T(theta_i),
// s_i = beta_{mc-1} * Yt[mc-1][i] (one rounding in T) and l = cols
template <typename T>
void eg_rotation(EgHost<T> &h, int mc, int cols, T beta_last, T *yt, size_t ldy, bool lock) {
    for (int c = 0; c < mc; ++c)
        for (size_t i = 0; i < ldy; ++i) yt[(size_t)c * ldy + i] = (int)i < cols && (int)i < mc ? (T)h.Y[(size_t)c * mc + h.wanted[i]] : T(0);
    if (!lock) return;
    for (int i = 0; i < cols; ++i) {
        h.theta_l[i] = (T)h.theta[h.wanted[i]];
        h.s_l[i] = beta_last * yt[(size_t)(mc - 1) * ldy + i];
    }
    h.l = cols;
}

}  // namespace smh
