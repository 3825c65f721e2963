// tools/sym_eigen_rr_host_check.cpp — the round-robin order of csim_sym_eigen_ordered (csrc/sym_eigen.cpp,
// csrc/sym_eigen.hpp) as a stand-alone program, for a run under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU
// (tools/obsop_sanitize.sh): the pairing takes every pair exactly once per sweep (n = 1 .. 66, 255, 256) in disjoint
// slots; residual, orthogonality, ordering and sign rule in that order; order 0 is csim::sym_eigen bit for bit; the
// storage forms the device launcher chooses; what is refused.  Prints "sym_eigen rr host check ok" and returns 0, or
// says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "sym_eigen.hpp"

#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            return 1;                                                  \
        }                                                              \
    } while (0)

using Matrix = std::vector<double>;

static Matrix gram_of(int n, int cols, std::mt19937_64& gen) {
    std::normal_distribution<double> normal;
    Matrix B(static_cast<size_t>(n) * cols), A(static_cast<size_t>(n) * n, 0.0);
    for (double& v : B) v = normal(gen);
    for (int p = 0; p < n; ++p)
        for (int q = p; q < n; ++q) {
            double s = 0.0;
            for (int c = 0; c < cols; ++c) s += B[static_cast<size_t>(p) * cols + c] * B[static_cast<size_t>(q) * cols + c];
            A[static_cast<size_t>(p) * n + q] = A[static_cast<size_t>(q) * n + p] = s;
        }
    return A;
}

static double frobenius(const Matrix& a) {
    double s = 0.0;
    for (double v : a) s += v * v;
    return std::sqrt(s);
}

static bool same_bits(const Matrix& a, const Matrix& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0;
}

static int pairing(int n) {
    const int m = n + (n & 1);
    std::vector<int> seen(static_cast<size_t>(m) * m, 0);
    for (int t = 0; t + 1 < m; ++t) {
        std::vector<int> used(m, 0);
        for (int k = 0; k < m / 2; ++k) {
            int p = -1, q = -1;
            csim::eigen_rr_pair(m, t, k, &p, &q);
            EXPECT(0 <= p && p < q && q < m);
            EXPECT(!used[p] && !used[q]);  // the slots of a step are disjoint
            used[p] = used[q] = 1;
            ++seen[static_cast<size_t>(p) * m + q];
            if (q >= n) EXPECT(k == 0 && p == t);  // the idle slot of an odd n is slot 0, its lone index t
        }
    }
    for (int p = 0; p < m; ++p)
        for (int q = 0; q < m; ++q) EXPECT(seen[static_cast<size_t>(p) * m + q] == (p < q ? 1 : 0));
    return 0;
}

// tolerances as in tools/sym_eigen_host_check.cpp: c n eps with c = 64
static int check(int n, const Matrix& A, const char* what) {
    const size_t N = static_cast<size_t>(n);
    Matrix lam(N), V(N * N), lam0(N), V0(N * N), lam1(N), V1(N * N);
    int sweeps = -1, sweeps0 = -1, sweeps1 = -1;
    EXPECT(csim::sym_eigen_ordered(n, A.data(), csim::EIGEN_ROUND_ROBIN, lam.data(), V.data(), &sweeps));
    EXPECT(sweeps >= 0 && sweeps < csim::SYM_EIGEN_MAX_SWEEPS);
    EXPECT(csim::sym_eigen_ordered(n, A.data(), csim::EIGEN_ROWS, lam0.data(), V0.data(), &sweeps0));
    EXPECT(csim::sym_eigen(n, A.data(), lam1.data(), V1.data(), &sweeps1));
    EXPECT(sweeps0 == sweeps1 && same_bits(lam0, lam1) && same_bits(V0, V1));
    const double tol = 64.0 * n * std::numeric_limits<double>::epsilon();
    Matrix res(N * N), orth(N * N);
    for (size_t p = 0; p < N; ++p)
        for (size_t r = 0; r < N; ++r) {
            double av = 0.0, vv = 0.0;
            for (size_t q = 0; q < N; ++q) av += A[p * N + q] * V[q * N + r], vv += V[q * N + p] * V[q * N + r];
            res[p * N + r] = av - V[p * N + r] * lam[r];
            orth[p * N + r] = vv - (p == r ? 1.0 : 0.0);
        }
    const double norm = frobenius(A);
    if (!(frobenius(res) <= tol * (norm > 0.0 ? norm : 1.0)) || !(frobenius(orth) <= tol)) {
        std::printf("FAILED %s n=%d: residual %.3g orthogonality %.3g tol %.3g\n", what, n,
                    frobenius(res) / (norm > 0.0 ? norm : 1.0), frobenius(orth), tol);
        return 1;
    }
    for (size_t r = 0; r + 1 < N; ++r) EXPECT(lam[r] >= lam[r + 1]);
    for (size_t r = 0; r < N; ++r) {
        size_t big = 0;
        for (size_t j = 1; j < N; ++j)
            if (std::fabs(V[j * N + r]) > std::fabs(V[big * N + r])) big = j;
        EXPECT(V[big * N + r] > 0.0);
    }
    return 0;
}

int main() {
    for (int n = 1; n <= 66; ++n)
        if (pairing(n)) return 1;
    if (pairing(255) || pairing(256)) return 1;
    std::mt19937_64 gen(2025);
    for (int n : {1, 2, 3, 4, 5, 17, 63, 64, 65, 100, 255, 256}) {
        if (check(n, gram_of(n, n + 3, gen), "random")) return 1;
        if (n >= 3 && check(n, gram_of(n, 2, gen), "rank 2")) return 1;
        if (n >= 3 && check(n, gram_of(n, 1, gen), "rank 1")) return 1;
        if (check(n, Matrix(static_cast<size_t>(n) * n, 0.0), "zero")) return 1;
    }
    {
        const double big = 1e150, tiny = 1e-150;
        if (check(2, {big, tiny, tiny, -big}, "wide range")) return 1;
        if (check(3, {tiny, tiny, 0.0, tiny, tiny, tiny, 0.0, tiny, tiny}, "tiny")) return 1;
    }
    // ties keep the lower original index first
    {
        const Matrix A = {1.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 1.0};
        Matrix lam(3), V(9);
        int sweeps = -1;
        EXPECT(csim::sym_eigen_ordered(3, A.data(), csim::EIGEN_ROUND_ROBIN, lam.data(), V.data(), &sweeps) && sweeps == 0);
        EXPECT(lam[0] == 3.0 && lam[1] == 1.0 && lam[2] == 1.0);
        EXPECT(V[1 * 3 + 0] == 1.0 && V[0 * 3 + 1] == 1.0 && V[2 * 3 + 2] == 1.0);
    }
    // refused, and nothing written
    {
        Matrix A = gram_of(3, 5, gen), lam(3, -7.0), V(9, -7.0);
        EXPECT(!csim::sym_eigen_ordered(3, A.data(), 2, lam.data(), V.data(), nullptr));
        EXPECT(!csim::sym_eigen_ordered(3, A.data(), -1, lam.data(), V.data(), nullptr));
        A[2] = std::numeric_limits<double>::quiet_NaN();
        EXPECT(!csim::sym_eigen_ordered(3, A.data(), csim::EIGEN_ROUND_ROBIN, lam.data(), V.data(), nullptr));
        EXPECT(!csim::sym_eigen_ordered(0, A.data(), csim::EIGEN_ROUND_ROBIN, lam.data(), V.data(), nullptr));
        EXPECT(!csim::sym_eigen_ordered(csim::SYM_EIGEN_MAX_N + 1, A.data(), csim::EIGEN_ROUND_ROBIN, lam.data(), V.data(),
                                        nullptr));
        EXPECT(lam[0] == -7.0 && V[8] == -7.0);
    }
    // the forms of the device launcher: the working matrices fit the 160 KiB of LDS beside 8 KiB of slot parameters
    {
        const long lds = 152L * 1024;
        EXPECT(16L * csim::EIGEN_LDS_MAX_N * csim::EIGEN_LDS_MAX_N <= lds);
        EXPECT(8L * csim::EIGEN_MIXED_MAX_N * csim::EIGEN_MIXED_MAX_N <= lds);
        EXPECT(csim::eigen_device_form(csim::EIGEN_LDS_MAX_N, 0) == 1 && csim::eigen_device_form(csim::EIGEN_LDS_MAX_N + 1, 0) == 2);
        EXPECT(csim::eigen_device_form(csim::EIGEN_MIXED_MAX_N, 0) == 2 && csim::eigen_device_form(csim::EIGEN_MIXED_MAX_N + 1, 0) == 3);
        EXPECT(csim::eigen_device_form(256, 0) == 3 && csim::eigen_device_form(257, 0) == 0 && csim::eigen_device_form(0, 0) == 0);
        EXPECT(csim::eigen_device_form(csim::EIGEN_LDS_MAX_N + 1, 1) == 0 && csim::eigen_device_form(5, 3) == 3);
        EXPECT(csim::eigen_device_form(5, 4) == 0);
    }
    std::printf("sym_eigen rr host check ok\n");
    return 0;
}
