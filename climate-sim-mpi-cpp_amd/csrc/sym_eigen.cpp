// sym_eigen.cpp — csim_sym_eigen: the cyclic Jacobi method of include/csim.h, operation by operation as written there.
// No HIP headers, no contraction: C, C++ and Python callers get the same bits from the same input.
#include "sym_eigen.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

// every build of this file also passes -ffp-contract=off (csrc/Makefile, tools/obsop_sanitize.sh)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace csim {

namespace {

// one pair of a sweep: the decisions and the rotation of include/csim.h on a (kept symmetric) and v (row p is vector p)
inline void rotate_pair(double* a, double* v, size_t N, size_t p, size_t q) {
    const double apq = a[p * N + q];
    if (apq == 0.0) return;
    const double g = std::fabs(apq);
    const double app = a[p * N + p], aqq = a[q * N + q];
    if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
        a[p * N + q] = a[q * N + p] = 0.0;
        return;
    }
    double h = aqq - app;
    double t;
    if (std::fabs(h) + g == std::fabs(h)) {
        t = apq / h;
    } else {
        const double theta = (0.5 * h) / apq;
        t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / std::sqrt(t * t + 1.0);
    const double s = t * c;
    const double tau = s / (1.0 + c);
    h = t * apq;
    a[p * N + p] = app - h;
    a[q * N + q] = aqq + h;
    a[p * N + q] = a[q * N + p] = 0.0;
    for (size_t j = 0; j < N; ++j) {
        if (j == p || j == q) continue;
        const double x = a[p * N + j], y = a[q * N + j];  // a_jp, a_jq through the mirror: contiguous reads
        const double xn = x - s * (y + x * tau);
        const double yn = y + s * (x - y * tau);
        a[j * N + p] = a[p * N + j] = xn;
        a[j * N + q] = a[q * N + j] = yn;
    }
    for (size_t j = 0; j < N; ++j) {
        const double x = v[p * N + j], y = v[q * N + j];
        v[p * N + j] = x - s * (y + x * tau);
        v[q * N + j] = y + s * (x - y * tau);
    }
}

}  // namespace

bool sym_eigen(int n, const double* A, double* lambda, double* V, int* sweeps) {
    return sym_eigen_ordered(n, A, EIGEN_ROWS, lambda, V, sweeps);
}

bool sym_eigen_ordered(int n, const double* A, int order, double* lambda, double* V, int* sweeps) {
    if (order != EIGEN_ROWS && order != EIGEN_ROUND_ROBIN) return false;
    if (n < 1 || n > SYM_EIGEN_MAX_N || !A || !lambda || !V) return false;
    const size_t N = static_cast<size_t>(n);
    for (size_t k = 0; k < N * N; ++k)
        if (!std::isfinite(A[k])) return false;
    // a: the working matrix, kept symmetric entry by entry (the lower triangle mirrors the upper); v: the rotations,
    // stored transposed (row p is vector p), so that a rotation works on two contiguous rows
    std::vector<double> a(N * N), v(N * N, 0.0);
    for (size_t p = 0; p < N; ++p)
        for (size_t q = p; q < N; ++q) a[p * N + q] = a[q * N + p] = A[p * N + q];
    for (size_t p = 0; p < N; ++p) v[p * N + p] = 1.0;

    int done = 0;
    for (; done < SYM_EIGEN_MAX_SWEEPS; ++done) {
        bool diagonal = true;
        for (size_t p = 0; p + 1 < N && diagonal; ++p)
            for (size_t q = p + 1; q < N; ++q)
                if (a[p * N + q] != 0.0) {
                    diagonal = false;
                    break;
                }
        if (diagonal) break;
        if (order == EIGEN_ROWS) {
            for (size_t p = 0; p + 1 < N; ++p)
                for (size_t q = p + 1; q < N; ++q) rotate_pair(a.data(), v.data(), N, p, q);
        } else {
            // the slots of a step are disjoint and a slot's parameters come from entries that no other slot writes, so
            // taking the slots one after the other is the step of include/csim.h, block by block
            const int m = n + (n & 1);
            for (int t = 0; t + 1 < m; ++t)
                for (int k = 0; k < m / 2; ++k) {
                    int p = 0, q = 0;
                    eigen_rr_pair(m, t, k, &p, &q);
                    if (q < n) rotate_pair(a.data(), v.data(), N, static_cast<size_t>(p), static_cast<size_t>(q));
                }
        }
    }

    // descending, ties to the lower original index; then the sign rule
    std::vector<int> perm(N);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(),
                     [&](int x, int y) { return a[x * N + x] > a[y * N + y]; });
    for (size_t r = 0; r < N; ++r) {
        const size_t src = static_cast<size_t>(perm[r]);
        lambda[r] = a[src * N + src];
        size_t big = 0;
        for (size_t j = 1; j < N; ++j)
            if (std::fabs(v[src * N + j]) > std::fabs(v[src * N + big])) big = j;
        const bool flip = v[src * N + big] < 0.0;
        for (size_t j = 0; j < N; ++j) V[j * N + r] = flip ? -v[src * N + j] : v[src * N + j];
    }
    if (sweeps) *sweeps = done;
    return true;
}

}  // namespace csim
