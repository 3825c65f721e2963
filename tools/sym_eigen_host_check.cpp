// tools/sym_eigen_host_check.cpp — the eigensolver of csim_sym_eigen (csrc/sym_eigen.cpp) as a stand-alone program, for
// a run under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU (tools/obsop_sanitize.sh): residual,
// orthogonality, ordering and sign rule on random, rank-deficient and repeated-eigenvalue matrices at every n of a
// list that ends at the limit, and what is refused.  Prints "sym_eigen host check ok" and returns 0, or says what
// failed and returns 1.
#include <cmath>
#include <cstdio>
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

// A = B B^T with B n x cols: rank min(n, cols)
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

// Q diag(d) Q^T with Q the vectors of a random matrix's decomposition: prescribed, possibly repeated, eigenvalues
static bool with_spectrum(int n, const std::vector<double>& d, std::mt19937_64& gen, Matrix* out) {
    const Matrix R = gram_of(n, n + 2, gen);
    Matrix lam(n), Q(static_cast<size_t>(n) * n);
    if (!csim::sym_eigen(n, R.data(), lam.data(), Q.data(), nullptr)) return false;
    out->assign(static_cast<size_t>(n) * n, 0.0);
    for (int p = 0; p < n; ++p)
        for (int q = p; q < n; ++q) {
            double s = 0.0;
            for (int r = 0; r < n; ++r) s += Q[static_cast<size_t>(p) * n + r] * d[r] * Q[static_cast<size_t>(q) * n + r];
            (*out)[static_cast<size_t>(p) * n + q] = (*out)[static_cast<size_t>(q) * n + p] = s;
        }
    return true;
}

static double frobenius(const Matrix& a) {
    double s = 0.0;
    for (double v : a) s += v * v;
    return std::sqrt(s);
}

// the checks of one matrix; tolerances c n eps with c = 64: Jacobi's backward error is a small multiple of n eps per
// sweep and the solver makes at most a dozen sweeps at these sizes
static int check(int n, const Matrix& A, const char* what) {
    const size_t N = static_cast<size_t>(n);
    Matrix lam(N), V(N * N);
    int sweeps = -1;
    EXPECT(csim::sym_eigen(n, A.data(), lam.data(), V.data(), &sweeps));
    EXPECT(sweeps >= 0 && sweeps < csim::SYM_EIGEN_MAX_SWEEPS);
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
    std::mt19937_64 gen(2024);
    for (int n : {1, 2, 3, 5, 17, 64, 100, 256}) {
        if (check(n, gram_of(n, n + 3, gen), "random")) return 1;
        if (n >= 3 && check(n, gram_of(n, 2, gen), "rank 2")) return 1;
        if (n >= 3 && n <= 100) {
            std::vector<double> d(n, 2.0);
            d[0] = 4.0, d[n - 1] = 1.0;
            Matrix A;
            EXPECT(with_spectrum(n, d, gen, &A));
            if (check(n, A, "repeated")) return 1;
        }
        if (check(n, Matrix(static_cast<size_t>(n) * n, 0.0), "zero")) return 1;
    }
    // ties keep the lower original index first; only the upper triangle is read
    {
        const Matrix A = {1.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 1.0};
        Matrix lam(3), V(9);
        int sweeps = -1;
        EXPECT(csim::sym_eigen(3, A.data(), lam.data(), V.data(), &sweeps) && sweeps == 0);
        EXPECT(lam[0] == 3.0 && lam[1] == 1.0 && lam[2] == 1.0);
        EXPECT(V[1 * 3 + 0] == 1.0 && V[0 * 3 + 1] == 1.0 && V[2 * 3 + 2] == 1.0);
        Matrix Bm = gram_of(4, 6, gen), C = Bm, l1(4), l2(4), V1(16), V2(16);
        for (int p = 1; p < 4; ++p)
            for (int q = 0; q < p; ++q) C[p * 4 + q] = 99.0;
        EXPECT(csim::sym_eigen(4, Bm.data(), l1.data(), V1.data(), nullptr));
        EXPECT(csim::sym_eigen(4, C.data(), l2.data(), V2.data(), nullptr));
        EXPECT(l1 == l2 && V1 == V2);
    }
    // refused, and nothing written
    {
        Matrix A = gram_of(3, 5, gen), lam(3, -7.0), V(9, -7.0);
        A[2] = std::numeric_limits<double>::quiet_NaN();
        EXPECT(!csim::sym_eigen(3, A.data(), lam.data(), V.data(), nullptr));
        A[2] = std::numeric_limits<double>::infinity();
        EXPECT(!csim::sym_eigen(3, A.data(), lam.data(), V.data(), nullptr));
        EXPECT(!csim::sym_eigen(0, A.data(), lam.data(), V.data(), nullptr));
        EXPECT(!csim::sym_eigen(csim::SYM_EIGEN_MAX_N + 1, A.data(), lam.data(), V.data(), nullptr));
        EXPECT(lam[0] == -7.0 && V[8] == -7.0);
    }
    // entries at the ends of the range: no overflow in the rotation, no endless sweeps
    {
        const double big = 1e150, tiny = 1e-150;
        if (check(2, {big, tiny, tiny, -big}, "wide range")) return 1;
        if (check(3, {tiny, tiny, 0.0, tiny, tiny, tiny, 0.0, tiny, tiny}, "tiny")) return 1;
    }
    std::printf("sym_eigen host check ok\n");
    return 0;
}
