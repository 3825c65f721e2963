// test_impact_global.cpp — the ensemble-space dot and the global forecast impact through climate::Ensemble
// (include/climate/ensemble.hpp) on a GPU, held against the C entry points on a twin that takes the same calls: dot
// against csim_ensemble_dot and, for member fields, against gram; obs_impact_global after an ETKF against
// csim_ensemble_obs_impact_global and against csim_obs_impact_global_value on the downloaded capture-time members;
// errors.  Prints "impact_global ok" and returns 0, or says what failed and returns 1.
#include <cmath>
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
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0;
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main() {
    const int B = 6, t = 2, M = B - 1, nx = 13, ny = 9, nx2 = nx + 2, K = 3, bc[4] = {0, 0, 0, 0};
    const std::size_t cells = static_cast<std::size_t>(nx2) * (ny + 2);
    std::mt19937_64 gen(5);
    std::normal_distribution<double> normal;
    std::vector<double> X(B * cells), F(K * cells), w(cells);
    for (double& v : X) v = 3.0 + normal(gen);
    for (double& v : F) v = normal(gen);
    for (double& v : w) v = normal(gen);
    climate::Ensemble e(B, nx, ny, 1.0, 1.0, bc), other(B, nx, ny, 1.0, 1.0, bc);
    e.upload_all(X), other.upload_all(X);
    const std::vector<double> pD(B, 0.05), pdt(B, 0.1), pvx(B, 0.5), pvy(B, -0.25);
    e.set_physics(pD, pdt, pvx, pvy);
    // the C entry points on a twin
    csim_ensemble* eb = nullptr;
    EXPECT(csim_ensemble_create(B, nx, ny, 1, 1.0, 1.0, bc, 0.0, &eb) == CSIM_OK);
    EXPECT(csim_ensemble_upload_all(eb, X.data()) == CSIM_OK);
    EXPECT(csim_ensemble_set_physics(eb, pD.data(), pdt.data(), pvx.data(), pvy.data()) == CSIM_OK);

    // dot: the method is the C call
    for (int centered = 0; centered < 2; ++centered) {
        const std::vector<double> got = e.dot(F, K, t, centered != 0);
        std::vector<double> want(static_cast<std::size_t>(M) * K, -1.0);
        EXPECT(csim_ensemble_dot(eb, t, centered, K, F.data(), want.data()) == CSIM_OK);
        EXPECT(same_bits(got, want));
    }
    // the ghost ring of a field is not read
    std::vector<double> ghost = F;
    ghost[0] = NAN, ghost[cells - 1] = NAN;
    EXPECT(same_bits(e.dot(ghost, K, t), e.dot(F, K, t)));
    // the fields of the forecast members, not centered: the columns of gram
    std::vector<double> mine(static_cast<std::size_t>(M) * cells);
    for (int k = 0; k < M; ++k)
        std::copy(X.begin() + (k + (k >= t)) * cells, X.begin() + (k + (k >= t) + 1) * cells, mine.begin() + k * cells);
    EXPECT(same_bits(e.dot(mine, M, t, false), e.gram(t, false)));
    EXPECT(e.download_all() == X);
    EXPECT(throws([&] { e.dot(F, K + 1, t); }));                                 // the size does not fit
    EXPECT(throws([&] { e.dot(std::vector<double>(), 0, t); }));                 // K = 0
    EXPECT(throws([&] { e.dot(std::vector<double>(17 * cells, 0.0), 17, t); })); // K = 17
    EXPECT(throws([&] { e.dot(F, K, B); }));
    ghost = F, ghost[static_cast<std::size_t>(nx2) + 1] = INFINITY;
    EXPECT(throws([&] { e.dot(ghost, K, t); }));

    // the global impact after an ETKF
    const std::vector<int> i = {1, 13, 7, 4, 10, 7}, j = {1, 9, 5, 7, 2, 5};
    const std::vector<double> r = {0.5, 0.25, 1.0, 0.1, 0.7, 0.3};
    const std::size_t n = i.size();
    climate::ObsNetwork net = e.obs_network(i, j, r, 3.0, true, 1);
    climate::ObsNetwork foreign = other.obs_network(i, j, r, 3.0, true, 1);
    std::vector<double> y(n);
    for (double& v : y) v = 3.0 + normal(gen);
    net.set_values(y), foreign.set_values(y);
    csim_obs_network* nb = nullptr;
    EXPECT(csim_obs_network_create(eb, static_cast<int>(n), i.data(), j.data(), r.data(), 3.0, 1, 1, &nb) == CSIM_OK);
    EXPECT(csim_obs_network_set_values(nb, y.data()) == CSIM_OK);
    EXPECT(csim_ensemble_obs_impact_global(eb, nb, w.data(), nullptr, nullptr) == CSIM_ERR_STATE);
    EXPECT(throws([&] { e.obs_impact_global(net, w); }));   // no capture
    std::vector<unsigned char> active(n, 1);
    active[3] = 0;
    net.set_active(active);
    e.assimilate_etkf(net, 1.1, t, true);
    net.impact_capture(t);
    EXPECT(csim_obs_network_set_active(nb, active.data()) == CSIM_OK);
    EXPECT(csim_ensemble_assimilate_etkf(eb, nb, 1.1, t, 1, 0.0) == CSIM_OK);
    EXPECT(csim_obs_network_impact_capture(nb, t) == CSIM_OK);
    EXPECT(csim_ensemble_run(eb, 3) == CSIM_OK);
    const climate::ObsValues v = net.fetch(false, true);
    const std::vector<double> A = e.download_all();
    e.run(3);
    const std::vector<double> Xf = e.download_all();
    const climate::ObsImpact got = e.obs_impact_global(net, w);
    EXPECT(e.download_all() == Xf);
    std::vector<double> J(n, -1.0);
    csim_obs_impact_summary sm{};
    EXPECT(csim_ensemble_obs_impact_global(eb, nb, w.data(), J.data(), &sm) == CSIM_OK);
    EXPECT(same_bits(got.impact, J) && got.summary.used == sm.used && got.summary.beneficial == sm.beneficial);
    EXPECT(same_bits(got.summary.total, sm.total) && sm.used == 5);
    // and the definition, from dot and the helper
    const std::vector<double> g = e.dot(w, 1, t);
    long long beneficial = 0;
    double total = 0.0;
    for (std::size_t o = 0; o < n; ++o) {
        double want = 0.0;
        if (active[o]) {
            auto at = [&](int k) {
                return A[static_cast<std::size_t>(k + (k >= t)) * cells + static_cast<std::size_t>(j[o]) * nx2 + i[o]];
            };
            double s = 0.0, pert[M];
            for (int k = 0; k < M; ++k) s = s + at(k);
            const double ha = s / M;
            for (int k = 0; k < M; ++k) pert[k] = at(k) - ha;
            EXPECT(csim_obs_impact_global_value(M, pert, g.data(), (y[o] - v.bg_mean[o]) / r[o], &want) == CSIM_OK);
        }
        EXPECT(same_bits(got.impact[o], want));
        beneficial += want < 0.0;
        total = total + want;  // one chunk
    }
    EXPECT(same_bits(got.impact[3], 0.0) && got.summary.beneficial == beneficial && same_bits(got.summary.total, total));
    EXPECT(!same_bits(e.obs_impact(net, w).impact, got.impact));   // the localised one is another estimate

    EXPECT(throws([&] { e.obs_impact_global(net, std::vector<double>(cells - 1, 0.0)); }));
    std::vector<double> bad = w;
    bad[static_cast<std::size_t>(3) * nx2 + 4] = NAN;
    EXPECT(throws([&] { e.obs_impact_global(net, bad); }));
    bad = w, bad[0] = NAN;  // the ghost ring is not read
    EXPECT(same_bits(e.obs_impact_global(net, bad).impact, got.impact));
    EXPECT(throws([&] { other.obs_impact_global(net, w); }));      // a network of another ensemble
    EXPECT(throws([&] { other.obs_impact_global(foreign, w); }));  // nothing captured there
    double out = 7.0;
    EXPECT(csim_obs_impact_global_value(1, g.data(), g.data(), 1.0, &out) == CSIM_ERR_ARG && out == 7.0);
    EXPECT(csim_ensemble_destroy(eb) == CSIM_OK);
    std::printf("impact_global ok\n");
    return 0;
}
