// tools/etkf_host_check.cpp — the host mathematics of the ETKF (csrc/etkf_weights.cpp on csrc/sym_eigen.cpp:
// csim_etkf_weights and csim_obs_gram_plan) as a stand-alone program, for a run under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU (tools/obsop_sanitize.sh).  No device, no HIP, nothing loaded into another
// process.  The weights of random observation-space Gram matrices at every M of a list that ends at the limit: the
// residual of (kappa I + C) Pa = I with Pa = W W / (M - 1), W symmetric bit for bit, W 1 = inflation 1, wbar against
// Pa c, gamma and dfs; the plan against brute force; and what is refused.  Prints "etkf host check ok" and returns 0,
// or says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "csim.h"

namespace csim {
static std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace csim

#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            return 1;                                                  \
        }                                                              \
    } while (0)

using Matrix = std::vector<double>;

// A = Z^T Z of nobs rows z = ((h_k - hb) / sr, (y - hb) / sr): what csim_ensemble_obs_gram sums, in plain order
static Matrix obs_gram(int M, int nobs, std::mt19937_64& gen) {
    std::normal_distribution<double> normal;
    std::uniform_real_distribution<double> var(0.5, 2.0);
    const size_t ma = static_cast<size_t>(M) + 1;
    Matrix A(ma * ma, 0.0), z(ma);
    for (int q = 0; q < nobs; ++q) {
        double s = 0.0;
        for (int k = 0; k < M; ++k) s += z[k] = 3.0 + normal(gen);
        const double hb = s / M, sr = std::sqrt(var(gen));
        for (int k = 0; k < M; ++k) z[k] = (z[k] - hb) / sr;
        z[M] = (3.0 + normal(gen) - hb) / sr;
        for (size_t a = 0; a < ma; ++a)
            for (size_t b = 0; b < ma; ++b) A[a * ma + b] += z[a] * z[b];
    }
    return A;
}

static int check(int M, int nobs, double inflation, std::mt19937_64& gen) {
    const size_t m = static_cast<size_t>(M), ma = m + 1;
    const Matrix A = obs_gram(M, nobs, gen);
    Matrix W(m * m), wbar(m), gamma(m);
    double dfs = -1.0;
    int sweeps = -1;
    EXPECT(csim_etkf_weights(M, A.data(), inflation, W.data(), wbar.data(), gamma.data(), &dfs, &sweeps) == CSIM_OK);
    EXPECT(sweeps >= 0 && sweeps < CSIM_SYM_EIGEN_MAX_SWEEPS);
    const double kappa = (M - 1) / (inflation * inflation), eps = std::numeric_limits<double>::epsilon();
    double cnorm = 0.0;
    for (size_t a = 0; a < m; ++a)
        for (size_t b = 0; b < m; ++b) cnorm = std::fmax(cnorm, std::fabs(A[a * ma + b]));
    // tolerances c M eps relative to the scale of (kappa I + C): Jacobi's backward error, as tools/sym_eigen_host_check.cpp
    const double tol = 64.0 * M * eps * (1.0 + cnorm / kappa);
    Matrix Pa(m * m);
    for (size_t a = 0; a < m; ++a)
        for (size_t b = 0; b < m; ++b) {
            EXPECT(W[a * m + b] == W[b * m + a]);
            double s = 0.0;
            for (size_t k = 0; k < m; ++k) s += W[a * m + k] * W[k * m + b];
            Pa[a * m + b] = s / (M - 1);
        }
    double dsum = 0.0;
    for (size_t a = 0; a < m; ++a) {
        double row = 0.0, pc = 0.0;
        for (size_t b = 0; b < m; ++b) {
            double s = kappa * Pa[a * m + b];
            for (size_t k = 0; k < m; ++k) s += A[a * ma + k] * Pa[k * m + b];
            const double res = s - (a == b ? 1.0 : 0.0);
            if (!(std::fabs(res) <= tol)) {
                std::printf("FAILED M=%d nobs=%d: residual %.3g at (%zu, %zu), tol %.3g\n", M, nobs, res, a, b, tol);
                return 1;
            }
            row += W[a * m + b];
            pc += Pa[a * m + b] * A[b * ma + m];
        }
        EXPECT(std::fabs(row - inflation) <= tol * inflation);
        EXPECT(std::fabs(wbar[a] - pc) <= tol * (1.0 + std::fabs(pc)));
        EXPECT(gamma[a] >= 0.0 && (a == 0 || gamma[a] <= gamma[a - 1]));
        dsum += gamma[a] / (kappa + gamma[a]);
    }
    EXPECT(std::fabs(dfs - dsum) <= tol * M && dfs >= 0.0 && dfs <= std::fmin(M - 1, nobs) + tol * M);
    // every output is optional
    EXPECT(csim_etkf_weights(M, A.data(), inflation, nullptr, nullptr, nullptr, nullptr, nullptr) == CSIM_OK);
    return 0;
}

static int check_plan() {
    for (int M : {2, 3, 64, 65, 128, 129, 256})
        for (int nobs : {1, 63, 64, 65, 4095, 4096, 4097, 16384, 16385, 65536, 65537, 1 << 20}) {
            long nseg = -1;
            int classes = -1;
            EXPECT(csim_obs_gram_plan(M, nobs, &nseg, &classes) == CSIM_OK);
            long segs = 0;
            for (long q = 0; q < nobs; q += 64) ++segs;
            const long cap = M <= 64 ? 1024 : M <= 128 ? 256 : 64;
            EXPECT(nseg == segs && classes == (segs < cap ? segs : cap));
            // every segment belongs to exactly one class, and no class is empty
            std::vector<int> owner(static_cast<size_t>(segs), -1), count(static_cast<size_t>(classes), 0);
            for (int g = 0; g < classes; ++g)
                for (long q = g; q < segs; q += classes) {
                    EXPECT(owner[static_cast<size_t>(q)] == -1);
                    owner[static_cast<size_t>(q)] = g, ++count[static_cast<size_t>(g)];
                }
            for (int v : owner) EXPECT(v >= 0);
            for (int v : count) EXPECT(v >= 1);
        }
    EXPECT(csim_obs_gram_plan(8, 100, nullptr, nullptr) == CSIM_OK);
    EXPECT(csim_obs_gram_plan(1, 100, nullptr, nullptr) == CSIM_ERR_ARG);
    EXPECT(csim_obs_gram_plan(8, 0, nullptr, nullptr) == CSIM_ERR_ARG);
    EXPECT(csim_obs_gram_plan(257, 100, nullptr, nullptr) == CSIM_ERR_UNSUPPORTED);
    return 0;
}

int main() {
    std::mt19937_64 gen(2025);
    for (int M : {2, 3, 5, 17, 64, 100, 256})
        for (double inflation : {1.0, 1.1}) {
            if (check(M, 40, inflation, gen)) return 1;
            if (check(M, 1, inflation, gen)) return 1;
            if (M <= 100 && check(M, 3 * M, inflation, gen)) return 1;
        }
    // no observation: W = inflation I, wbar = 0
    {
        const int M = 4;
        Matrix A(25, 0.0), W(16), wbar(4), gamma(4);
        double dfs = -1.0;
        EXPECT(csim_etkf_weights(M, A.data(), 1.5, W.data(), wbar.data(), gamma.data(), &dfs, nullptr) == CSIM_OK);
        for (int a = 0; a < M; ++a)
            for (int b = 0; b < M; ++b) EXPECT(std::fabs(W[a * M + b] - (a == b ? 1.5 : 0.0)) <= 4e-16);
        EXPECT(dfs == 0.0 && wbar[0] == 0.0 && wbar[3] == 0.0 && gamma[0] == 0.0);
    }
    // refused, and nothing written
    {
        Matrix A = obs_gram(3, 10, gen), W(9, -7.0);
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        EXPECT(csim_etkf_weights(1, A.data(), 1.0, W.data(), nullptr, nullptr, nullptr, nullptr) == CSIM_ERR_ARG);
        EXPECT(csim_etkf_weights(257, A.data(), 1.0, W.data(), nullptr, nullptr, nullptr, nullptr) ==
               CSIM_ERR_UNSUPPORTED);
        for (double bad : {0.999, -2.0, nan, inf})
            EXPECT(csim_etkf_weights(3, A.data(), bad, W.data(), nullptr, nullptr, nullptr, nullptr) == CSIM_ERR_ARG);
        EXPECT(csim_etkf_weights(3, nullptr, 1.0, W.data(), nullptr, nullptr, nullptr, nullptr) == CSIM_ERR_ARG);
        for (size_t at : {size_t(1), size_t(3), size_t(12), size_t(15)})
            for (double bad : {nan, inf}) {
                Matrix Bm = A;
                Bm[at] = bad;
                EXPECT(csim_etkf_weights(3, Bm.data(), 1.0, W.data(), nullptr, nullptr, nullptr, nullptr) ==
                       CSIM_ERR_ARG);
            }
        EXPECT(W[0] == -7.0 && W[8] == -7.0);
    }
    if (check_plan()) return 1;
    std::printf("etkf host check ok\n");
    return 0;
}
