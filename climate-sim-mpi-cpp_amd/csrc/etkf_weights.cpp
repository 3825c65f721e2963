// etkf_weights.cpp — csim_etkf_weights and csim_obs_gram_plan: the symmetric square-root ETKF in ensemble space,
// operation by operation as include/csim.h writes it, on top of sym_eigen.cpp.  No HIP headers, no contraction: C, C++
// and Python callers get the same bits from the same input.
#include "gram_plan.hpp"

#include <cmath>
#include <new>
#include <vector>

#include "obs_taps.hpp"
#include "sym_eigen.hpp"

// every build of this file also passes -ffp-contract=off (csrc/Makefile, tools/obsop_sanitize.sh)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

using namespace csim;

static_assert(ESPACE_MAX_MEMBERS == CSIM_ESPACE_MAX_MEMBERS && ESPACE_MAX_MEMBERS <= SYM_EIGEN_MAX_N,
              "the ETKF's limit is that of the ensemble space");

extern "C" {

int csim_obs_gram_plan(int M, int nobs, long* nseg, int* classes) {
    OBS_REQUIRE(M >= 2 && nobs >= 1, "M must be >= 2 and nobs >= 1");
    if (M > ESPACE_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_obs_gram_plan: at most CSIM_ESPACE_MAX_MEMBERS forecast members");
    if (nseg) *nseg = gram_segments(nobs);
    if (classes) *classes = gram_classes(M, nobs);
    return CSIM_OK;
}

int csim_etkf_weights(int M, const double* A, double inflation, double* W, double* wbar, double* gamma, double* dfs,
                      int* sweeps) {
    return csim_etkf_weights_ordered(M, A, inflation, CSIM_EIGEN_ROWS, W, wbar, gamma, dfs, sweeps);
}

int csim_etkf_weights_ordered(int M, const double* A, double inflation, int order, double* W, double* wbar,
                              double* gamma, double* dfs, int* sweeps) {
    OBS_REQUIRE(M >= 2, "M must be >= 2");
    if (M > ESPACE_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_etkf_weights: at most CSIM_ESPACE_MAX_MEMBERS forecast members");
    OBS_REQUIRE(std::isfinite(inflation) && inflation >= 1.0, "inflation must be finite and >= 1");
    OBS_REQUIRE(A, "null argument");
    OBS_REQUIRE(order == CSIM_EIGEN_ROWS || order == CSIM_EIGEN_ROUND_ROBIN, "order must be CSIM_EIGEN_ROWS or "
                                                                             "CSIM_EIGEN_ROUND_ROBIN");
    const size_t m = static_cast<size_t>(M), ma = m + 1;
    for (size_t k = 0; k < ma * ma; ++k) OBS_REQUIRE(std::isfinite(A[k]), "csim_etkf_weights: a non-finite entry of A");
    try {
        std::vector<double> C(m * m), lam(m), V(m * m), f(m), g(m), G(m), fu(m);
        for (size_t a = 0; a < m; ++a)
            for (size_t b = 0; b < m; ++b) C[a * m + b] = A[a * ma + b];
        int done = 0;
        OBS_REQUIRE(sym_eigen_ordered(M, C.data(), order, lam.data(), V.data(), &done),
                    "csim_etkf_weights: a non-finite entry of A");
        const double rho = inflation * inflation;
        const double kappa = static_cast<double>(M - 1) / rho;
        double d = 0.0;
        for (size_t r = 0; r < m; ++r) {
            G[r] = lam[r] > 0.0 ? lam[r] : 0.0;
            f[r] = 1.0 / (kappa + G[r]);
            g[r] = std::sqrt(static_cast<double>(M - 1) * f[r]);
            double u = 0.0;
            for (size_t a = 0; a < m; ++a) u = u + V[a * m + r] * A[a * ma + m];
            fu[r] = f[r] * u;
            d = d + G[r] * f[r];
        }
        if (wbar)
            for (size_t a = 0; a < m; ++a) {
                double s = 0.0;
                for (size_t r = 0; r < m; ++r) s = s + V[a * m + r] * fu[r];
                wbar[a] = s;
            }
        if (W)
            for (size_t a = 0; a < m; ++a)
                for (size_t b = a; b < m; ++b) {
                    double s = 0.0;
                    for (size_t r = 0; r < m; ++r) s = s + (V[a * m + r] * g[r]) * V[b * m + r];
                    W[a * m + b] = W[b * m + a] = s;
                }
        if (gamma)
            for (size_t r = 0; r < m; ++r) gamma[r] = G[r];
        if (dfs) *dfs = d;
        if (sweeps) *sweeps = done;
        return CSIM_OK;
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, "csim_etkf_weights: out of host memory");
    }
}

}  // extern "C"
