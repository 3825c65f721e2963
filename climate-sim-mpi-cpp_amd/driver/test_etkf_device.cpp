// test_etkf_device.cpp — the device ETKF through climate::Ensemble (include/climate/ensemble.hpp) on a GPU:
// climate::sym_eigen_batch against climate::sym_eigen in the round-robin order, and Ensemble::assimilate_etkf_device
// against the C entry point on a twin and against the composition obs_gram -> etkf_weights(round robin) -> transform on
// a third (the same bits), on one 37 x 21 case of 12 forecast members with 40 bilinear observations; etkf_info, and what
// is refused.  Prints "etkf device ok" and returns 0, or says what failed and returns 1.
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
    std::mt19937_64 gen(12);
    std::normal_distribution<double> normal;
    std::uniform_real_distribution<double> px(1.0, nx), py(1.0, ny), pr(0.5, 2.0);
    std::vector<double> X(static_cast<std::size_t>(B) * cells), x(nobs), y(nobs), r(nobs), vals(nobs);
    for (double& v : X) v = 2.0 + normal(gen);
    for (int o = 0; o < nobs; ++o) x[o] = px(gen), y[o] = py(gen), r[o] = pr(gen), vals[o] = 2.0 + normal(gen);
    std::vector<unsigned char> mask(nobs, 1);
    mask[3] = mask[17] = 0;

    climate::Ensemble a(B, nx, ny, 1.0, 1.0, bc), c(B, nx, ny, 1.0, 1.0, bc);
    a.upload_all(X), c.upload_all(X);
    const climate::ObsTaps taps = climate::Ensemble::bilinear_taps(nx, ny, x, y);
    climate::ObsNetwork na = a.obs_network(taps, r, 2.5, false, 2), nc = c.obs_network(taps, r, 2.5);
    na.set_values(vals), nc.set_values(vals);
    na.set_active(mask), nc.set_active(mask);
    csim_ensemble* eb = nullptr;
    csim_obs_network* nb = nullptr;
    EXPECT(csim_ensemble_create(B, nx, ny, 1, 1.0, 1.0, bc, 0.0, &eb) == CSIM_OK);
    EXPECT(csim_ensemble_upload_all(eb, X.data()) == CSIM_OK);
    EXPECT(csim_obs_network_create_linear(eb, nobs, taps.i.data(), taps.j.data(), taps.start.data(), taps.di.data(),
                                          taps.dj.data(), taps.w.data(), r.data(), 2.5, 0, 2, &nb) == CSIM_OK);
    EXPECT(csim_obs_network_set_values(nb, vals.data()) == CSIM_OK);
    EXPECT(csim_obs_network_set_active(nb, mask.data()) == CSIM_OK);

    // the composition on the third ensemble, in the round-robin order
    const climate::ObsGram g = c.obs_gram(nc, t);
    const climate::EtkfWeights w = climate::etkf_weights(g.A, M, inflation, CSIM_EIGEN_ROUND_ROBIN);
    const climate::EtkfWeights rows = climate::etkf_weights(g.A, M, inflation);
    EXPECT(same_bits(rows.W, climate::etkf_weights(g.A, M, inflation, CSIM_EIGEN_ROWS).W));
    c.transform(w.W, w.wbar, t);

    // the eigensolver alone: two matrices on the device against the host order
    std::vector<double> C2(2 * static_cast<std::size_t>(M) * M);
    for (int p = 0; p < M; ++p)
        for (int q = 0; q < M; ++q) {
            C2[p * M + q] = g.A[p * ma + q];
            C2[M * M + p * M + q] = p == q ? 1.0 + p : 0.0;
        }
    const climate::SymEigenBatch eb2 = climate::sym_eigen_batch(C2, M, 2);
    const std::vector<double> first(C2.begin(), C2.begin() + M * M);
    const climate::SymEigen host = climate::sym_eigen(first, M, CSIM_EIGEN_ROUND_ROBIN);
    EXPECT(eb2.status[0] == CSIM_EIGEN_OK && eb2.status[1] == CSIM_EIGEN_OK && eb2.sweeps[1] == 0);
    EXPECT(eb2.sweeps[0] == host.sweeps && host.sweeps > 0);
    EXPECT(std::memcmp(eb2.lambda.data(), host.lambda.data(), sizeof(double) * M) == 0);
    EXPECT(std::memcmp(eb2.V.data(), host.V.data(), sizeof(double) * M * M) == 0);
    EXPECT(eb2.lambda[M] == static_cast<double>(M) && eb2.lambda[2 * M - 1] == 1.0);
    int chosen = 0, most = 0;
    EXPECT(csim_sym_eigen_device_form(M, 0, &chosen, &most) == CSIM_OK && chosen == 1 && most == CSIM_SYM_EIGEN_MAX_N);

    // the analysis: the C++ method, the C entry point, the composition
    a.assimilate_etkf_device(na, inflation, t, true);
    EXPECT(csim_ensemble_assimilate_etkf_device(eb, nb, inflation, t, 1, 0.0) == CSIM_OK);
    const climate::EtkfAnalysis r1 = a.etkf_info(t);
    long long used = -1;
    double chi2 = -1.0, dfs = -1.0;
    std::vector<double> gamma(M);
    int ng = -1, sweeps = -1, status = -1;
    EXPECT(csim_ensemble_etkf_info2(eb, &used, &chi2, &dfs, gamma.data(), &ng, &sweeps, &status) == CSIM_OK);
    EXPECT(r1.n_used == used && used == g.n_used && used == nobs - 2 && r1.chi2 == chi2 && chi2 == g.A[ma * ma - 1]);
    EXPECT(r1.dfs == dfs && dfs == w.dfs && ng == M && same_bits(r1.gamma, gamma) && same_bits(gamma, w.gamma));
    EXPECT(r1.sweeps == sweeps && sweeps == w.sweeps && r1.status == status && status == CSIM_EIGEN_OK);
    long long used1 = -1;
    EXPECT(csim_ensemble_etkf_info(eb, &used1, nullptr, nullptr, nullptr, nullptr) == CSIM_OK && used1 == used);
    std::vector<double> Xa = a.download_all(), Xb(X.size());
    EXPECT(csim_ensemble_download_all(eb, Xb.data()) == CSIM_OK);
    EXPECT(same_bits(Xa, Xb) && same_bits(Xa, c.download_all()) && !same_bits(Xa, X));
    EXPECT(std::memcmp(&Xa[t * cells], &X[t * cells], sizeof(double) * cells) == 0);
    EXPECT(na.log().size() == 1 && na.screen_log().size() == 1 && na.screen_log()[0].n_inactive == 2.0);

    // refused
    climate::Ensemble other(B, nx, ny, 1.0, 1.0, bc);
    EXPECT(throws([&] { other.assimilate_etkf_device(na, 1.0, t); }));    // another ensemble's network
    EXPECT(throws([&] { other.etkf_info(t); }));                          // no analysis yet
    EXPECT(throws([&] { a.assimilate_etkf_device(na, 0.5, t); }));        // inflation < 1
    EXPECT(throws([&] { climate::sym_eigen(first, M, 2); }));             // unknown order
    EXPECT(throws([&] { climate::sym_eigen_batch(C2, M, 3); }));          // array size
    EXPECT(throws([&] { climate::etkf_weights(g.A, M, inflation, 7); }));
    EXPECT(same_bits(a.download_all(), Xa));

    EXPECT(csim_ensemble_destroy(eb) == CSIM_OK);
    std::printf("etkf device ok\n");
    return 0;
}
