// test_obsimpact.cpp — the forecast impact through climate::ObsNetwork / climate::Ensemble
// (include/climate/ensemble.hpp) on a GPU: impact_capture and obs_impact against the csim.h definition worked out here
// on the downloaded members with csim_obs_impact_fold and csim_ensemble_gc_table, bit for bit; a screened observation's
// +0; the capture across run() and a later unrecorded analysis; no side effects; errors; a handle that outlives its
// ensemble.  Prints "obsimpact ok" and returns 0, or says what failed and returns 1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main() {
    const int B = 6, t = 2, M = B - 1, nx = 40, ny = 24, nx2 = nx + 2, bc[4] = {0, 1, 2, 0};
    const std::size_t cells = static_cast<std::size_t>(nx2) * (ny + 2);
    std::mt19937_64 gen(11);
    std::normal_distribution<double> normal;
    std::vector<double> X(B * cells), w(cells);
    for (double& v : X) v = normal(gen);
    for (double& v : w) v = normal(gen);
    const std::vector<int> i = {1, 40, 20, 21, 7, 33, 12, 28}, j = {1, 24, 12, 13, 20, 5, 8, 17};
    const std::vector<double> r = {0.5, 0.25, 1.0, 0.1, 0.7, 0.3, 0.4, 0.6};
    const std::size_t n = i.size();
    const double loc = 3.0;
    int lx = 0, ly = 0;
    EXPECT(csim_ensemble_gc_table(1.0, 1.0, loc, nx, ny, &lx, &ly, nullptr) == CSIM_OK);
    std::vector<double> rho(static_cast<std::size_t>(2 * lx + 1) * (2 * ly + 1));
    EXPECT(csim_ensemble_gc_table(1.0, 1.0, loc, nx, ny, &lx, &ly, rho.data()) == CSIM_OK);

    auto a = std::make_unique<climate::Ensemble>(B, nx, ny, 1.0, 1.0, bc);
    climate::Ensemble b(B, nx, ny, 1.0, 1.0, bc);
    a->upload_all(X), b.upload_all(X);
    const std::vector<double> phys_D(B, 0.05), phys_dt(B, 0.1), phys_vx = {0.5, -0.3, 0.0, 0.2, -0.2, 0.1},
                              phys_vy = {-0.25, 0.4, 0.0, 0.2, -0.1, 0.3};
    a->set_physics(phys_D, phys_dt, phys_vx, phys_vy);
    climate::ObsNetwork net = a->obs_network(i, j, r, loc, true, 2);
    climate::ObsNetwork foreign = b.obs_network(i, j, r, loc, true, 1);
    std::vector<double> y(n);
    for (double& v : y) v = normal(gen);
    net.set_values(y), foreign.set_values(y);
    EXPECT(throws([&] { a->obs_impact(net, w); }));   // no capture
    EXPECT(throws([&] { net.impact_capture(t); }));   // no recorded analysis
    std::vector<unsigned char> active(n, 1);
    active[5] = 0;
    net.set_active(active);
    a->assimilate(net, 1.05, t, true);
    net.impact_capture(t);
    const climate::ObsValues v = net.fetch(false, true);
    const std::vector<double> A = a->download_all();
    a->run(3);
    const std::vector<double> F = a->download_all();
    const climate::ObsImpact got = a->obs_impact(net, w);
    EXPECT(a->download_all() == F);

    // the definition, on the host: forecast member k is member k + (k >= t)
    auto at = [&](const std::vector<double>& S, int k, int cj, int ci) {
        return S[static_cast<std::size_t>(k + (k >= t)) * cells + static_cast<std::size_t>(cj) * nx2 + ci];
    };
    long long beneficial = 0;
    double total = 0.0;
    for (std::size_t o = 0; o < n; ++o) {
        double want = 0.0;
        if (active[o]) {
            double s = 0.0, pert[M];
            for (int k = 0; k < M; ++k) s = s + at(A, k, j[o], i[o]);
            const double ha = s / M;
            for (int k = 0; k < M; ++k) pert[k] = at(A, k, j[o], i[o]) - ha;
            const double dn = (y[o] - v.bg_mean[o]) / r[o];
            const int i0 = std::max(1, i[o] - lx), i1 = std::min(nx, i[o] + lx), j0 = std::max(1, j[o] - ly),
                      j1 = std::min(ny, j[o] + ly);
            std::vector<double> u;
            for (int cj = j0; cj <= j1; ++cj)
                for (int ci = i0; ci <= i1; ++ci) {
                    const double rh = rho[static_cast<std::size_t>(cj - j[o] + ly) * (2 * lx + 1) + (ci - i[o] + lx)];
                    if (!(rh > 0.0)) {
                        u.push_back(0.0);
                        continue;
                    }
                    double sx = 0.0, c = 0.0;
                    for (int k = 0; k < M; ++k) sx = sx + at(F, k, cj, ci);
                    const double xbar = sx / M;
                    for (int k = 0; k < M; ++k) c = c + (at(F, k, cj, ci) - xbar) * pert[k];
                    u.push_back((rh * (c / (M - 1))) * w[static_cast<std::size_t>(cj) * nx2 + ci]);
                }
            double S = 0.0;
            EXPECT(csim_obs_impact_fold(u.data(), static_cast<long>(u.size()), &S) == CSIM_OK);
            want = dn * S;
        }
        EXPECT(same_bits(got.impact[o], want));
        beneficial += want < 0.0;
        total = total + want;  // one chunk
    }
    EXPECT(same_bits(got.impact[5], 0.0) && got.summary.used == 7 && got.summary.beneficial == beneficial);
    EXPECT(same_bits(got.summary.total, total) && beneficial > 0 && beneficial < 7);

    // new values and an unrecorded analysis leave the capture alone; a capture is refused while that analysis is the last
    for (double& val : y) val = normal(gen);
    net.set_values(y);
    a->assimilate(net, 1.0, t, false, 3.0);
    EXPECT(throws([&] { net.impact_capture(t); }));
    a->upload_all(F);
    EXPECT(a->obs_impact(net, w).impact == got.impact);
    // a new recorded analysis and capture give another result
    a->assimilate(net, 1.0, t, true);
    net.impact_capture(t);
    a->upload_all(F);
    EXPECT(a->obs_impact(net, w).impact != got.impact);

    EXPECT(throws([&] { a->obs_impact(net, std::vector<double>(cells - 1, 0.0)); }));
    std::vector<double> bad = w;
    bad[static_cast<std::size_t>(3) * nx2 + 4] = NAN;
    EXPECT(throws([&] { a->obs_impact(net, bad); }));
    bad = w, bad[0] = NAN;  // the ghost ring is not read
    EXPECT(a->obs_impact(net, bad).impact == a->obs_impact(net, w).impact);
    EXPECT(throws([&] { b.obs_impact(net, w); }));       // a network of another ensemble
    EXPECT(throws([&] { net.impact_capture(B); }));
    EXPECT(throws([&] { foreign.impact_capture(); }));   // nothing recorded there

    // a network that outlives its ensemble: every call throws, destroying it is safe
    a.reset();
    EXPECT(throws([&] { net.impact_capture(t); }));
    EXPECT(throws([&] { b.obs_impact(net, w); }));
    std::printf("obsimpact ok\n");
    return 0;
}
