// test_etkf.cpp — the ETKF through climate::Ensemble (include/climate/ensemble.hpp) on a GPU: Ensemble::obs_gram,
// climate::etkf_weights and Ensemble::assimilate_etkf against the C entry points on a twin (the same bits) on one
// 37 x 21 case of 12 forecast members with 40 bilinear observations, the composition behind the analysis, and what is
// refused.  Prints "etkf ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstring>
#include <random>

#include "climate/ensemble.hpp"

#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            return 1;                                                  \
        }                                                              \
    } while (0)

template <class F> static bool throws(F&& f) {
    try {
        f();
    } catch (const std::exception&) {
        return true;
    }
    return false;
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}

int main() {
    const int B = 13, t = 4, M = B - 1, nx = 37, ny = 21, nobs = 40, bc[4] = {0, 1, 2, 0};
    const double inflation = 1.1;
    const std::size_t cells = static_cast<std::size_t>(nx + 2) * (ny + 2), ma = M + 1;
    std::mt19937_64 gen(11);
    std::normal_distribution<double> normal;
    std::uniform_real_distribution<double> px(1.0, nx), py(1.0, ny), pr(0.5, 2.0);
    std::vector<double> X(static_cast<std::size_t>(B) * cells), x(nobs), y(nobs), r(nobs), vals(nobs);
    for (double& v : X) v = 2.0 + normal(gen);
    for (int o = 0; o < nobs; ++o) x[o] = px(gen), y[o] = py(gen), r[o] = pr(gen), vals[o] = 2.0 + normal(gen);
    std::vector<unsigned char> mask(nobs, 1);
    mask[3] = mask[17] = 0;

    // the C++ methods on one ensemble, the C entry points on its twin
    climate::Ensemble a(B, nx, ny, 1.0, 1.0, bc);
    a.upload_all(X);
    const climate::ObsTaps taps = climate::Ensemble::bilinear_taps(nx, ny, x, y);
    climate::ObsNetwork na = a.obs_network(taps, r, 2.5, false, 2);
    na.set_values(vals);
    na.set_active(mask);
    csim_ensemble* eb = nullptr;
    csim_obs_network* nb = nullptr;
    EXPECT(csim_ensemble_create(B, nx, ny, 1, 1.0, 1.0, bc, 0.0, &eb) == CSIM_OK);
    EXPECT(csim_ensemble_upload_all(eb, X.data()) == CSIM_OK);
    EXPECT(csim_obs_network_create_linear(eb, nobs, taps.i.data(), taps.j.data(), taps.start.data(), taps.di.data(),
                                          taps.dj.data(), taps.w.data(), r.data(), 2.5, 0, 2, &nb) == CSIM_OK);
    EXPECT(csim_obs_network_set_values(nb, vals.data()) == CSIM_OK);
    EXPECT(csim_obs_network_set_active(nb, mask.data()) == CSIM_OK);

    // the matrix
    std::vector<double> A(ma * ma), ll(M);
    long long used = -1;
    EXPECT(csim_ensemble_obs_gram(eb, nb, t, A.data(), ll.data(), &used) == CSIM_OK);
    const climate::ObsGram g = a.obs_gram(na, t, true);
    EXPECT(same_bits(g.A, A) && same_bits(g.loglik, ll) && g.n_used == used && used == nobs - 2);
    for (std::size_t p = 0; p < ma; ++p)
        for (std::size_t q = 0; q < ma; ++q) EXPECT(A[p * ma + q] == A[q * ma + p] && (p != q || A[p * ma + q] > 0.0));
    EXPECT(a.obs_gram(na, t).loglik.empty());
    EXPECT(csim_ensemble_obs_gram(eb, nb, t, nullptr, nullptr, nullptr) == CSIM_OK);
    long nseg = 0;
    int classes = 0;
    EXPECT(csim_obs_gram_plan(M, nobs, &nseg, &classes) == CSIM_OK && nseg == 1 && classes == 1);

    // the weights
    const climate::EtkfWeights w = climate::etkf_weights(A, M, inflation);
    std::vector<double> W(static_cast<std::size_t>(M) * M), wbar(M), gamma(M);
    double dfs = -1.0;
    int sweeps = -1;
    EXPECT(csim_etkf_weights(M, A.data(), inflation, W.data(), wbar.data(), gamma.data(), &dfs, &sweeps) == CSIM_OK);
    EXPECT(same_bits(w.W, W) && same_bits(w.wbar, wbar) && same_bits(w.gamma, gamma) && w.dfs == dfs);
    EXPECT(w.sweeps == sweeps && sweeps > 0 && dfs > 0.0 && dfs < M - 1);
    for (int p = 0; p < M; ++p)
        for (int q = 0; q < M; ++q) EXPECT(W[p * M + q] == W[q * M + p]);

    // the analysis: the C++ method, the C entry point, and the composition through the public calls on a third
    climate::Ensemble c(B, nx, ny, 1.0, 1.0, bc);
    c.upload_all(X);
    c.transform(W, wbar, t);
    const climate::EtkfAnalysis r1 = a.assimilate_etkf(na, inflation, t, true);
    EXPECT(csim_ensemble_assimilate_etkf(eb, nb, inflation, t, 1, 0.0) == CSIM_OK);
    long long used2 = -1;
    double chi2 = -1.0, dfs2 = -1.0;
    std::vector<double> gamma2(M);
    int ng = -1;
    EXPECT(csim_ensemble_etkf_info(eb, &used2, &chi2, &dfs2, gamma2.data(), &ng) == CSIM_OK);
    EXPECT(r1.n_used == used2 && used2 == used && r1.chi2 == chi2 && chi2 == A[ma * ma - 1] && r1.dfs == dfs2 &&
           dfs2 == dfs && ng == M && same_bits(r1.gamma, gamma2) && same_bits(gamma2, gamma));
    std::vector<double> Xa = a.download_all(), Xb(X.size());
    EXPECT(csim_ensemble_download_all(eb, Xb.data()) == CSIM_OK);
    EXPECT(same_bits(Xa, Xb) && same_bits(Xa, c.download_all()) && !same_bits(Xa, X));
    EXPECT(std::memcmp(&Xa[t * cells], &X[t * cells], sizeof(double) * cells) == 0);
    EXPECT(na.log().size() == 1 && na.screen_log().size() == 1 && na.screen_log()[0].n_inactive == 2.0);
    const std::vector<unsigned char> st = na.status();
    EXPECT(st[3] == CSIM_OBS_INACTIVE && st[17] == CSIM_OBS_INACTIVE && st[0] == CSIM_OBS_USED);

    // refused
    climate::Ensemble other(B, nx, ny, 1.0, 1.0, bc);
    EXPECT(throws([&] { other.obs_gram(na, t); }));                        // another ensemble's network
    EXPECT(throws([&] { other.assimilate_etkf(na, 1.0, t); }));
    EXPECT(throws([&] { a.assimilate_etkf(na, 0.5, t); }));                // inflation < 1
    EXPECT(throws([&] { a.obs_gram(na, B); }));
    EXPECT(throws([&] { climate::etkf_weights(A, M - 1); }));              // array size
    EXPECT(throws([&] { climate::etkf_weights(A, M, 0.9); }));
    EXPECT(throws([&] { climate::etkf_weights({0.0, 0.0, 0.0, 0.0}, 1); }));
    climate::ObsNetwork empty = a.obs_network(taps, r, 2.5);
    EXPECT(throws([&] { a.obs_gram(empty, t); }));                         // no values yet
    EXPECT(same_bits(a.download_all(), Xa));

    EXPECT(csim_ensemble_destroy(eb) == CSIM_OK);
    std::printf("etkf ok\n");
    return 0;
}
