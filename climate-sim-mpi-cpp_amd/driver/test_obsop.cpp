// test_obsop.cpp — linear observations through the C++ surface (include/climate/ensemble.hpp) on a GPU: a bilinear
// network built from fractional positions, one recorded analysis, the log.  The operator is checked against a host
// loop over the downloaded members, the builders against their definition.  Prints "obsop ok" and returns 0, or says
// what failed and returns 1.
#include <cmath>
#include <cstdio>
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

int main() {
    const int B = 6, nx = 40, ny = 24, bc[4] = {0, 1, 2, 0}, t = 2;
    std::mt19937_64 gen(7);
    std::normal_distribution<double> normal;
    const std::size_t cells = static_cast<std::size_t>(nx + 2) * (ny + 2);
    std::vector<double> X(B * cells);
    for (double& v : X) v = normal(gen);
    const std::vector<double> x = {1.0, 40.0, 20.25, 21.5, 7.75, 33.125}, y = {1.0, 24.0, 12.5, 13.0, 20.875, 5.25};
    const std::vector<double> r = {0.5, 0.25, 1.0, 0.1, 0.7, 0.3};

    const climate::ObsTaps taps = climate::Ensemble::bilinear_taps(nx, ny, x, y);
    EXPECT(taps.size() == 6 && taps.start.back() == 24 && taps.w.size() == 24);
    EXPECT(taps.i[1] == 39 && taps.j[1] == 23 && taps.w[4 + 3] == 1.0);   // x == nx: all weight on the last column
    EXPECT(taps.i[2] == 20 && taps.j[2] == 12 && taps.w[8] == 0.75 * 0.5 && taps.w[11] == 0.25 * 0.5);
    const climate::ObsTaps box = climate::Ensemble::box_taps(nx, ny, {1, 20}, {1, 12}, 1, 1);
    EXPECT(box.start[1] == 4 && box.start[2] == 13 && box.w[0] == 0.25 && box.w[4] == 1.0 / 9.0);
    EXPECT(throws([&] { climate::Ensemble::box_taps(nx, ny, {20}, {12}, 4, 4); }));
    EXPECT(throws([&] { climate::Ensemble::bilinear_taps(nx, ny, {0.5}, {1.0}); }));

    climate::Ensemble e(B, nx, ny, 1.0, 1.0, bc);
    e.upload_all(X);
    climate::ObsNetwork net = e.obs_network(taps, r, 3.0, false, 1);
    EXPECT(net.size() == 6 && net.taps() == 24 && net.levels() >= 1);
    climate::ObsNetwork points = e.obs_network(taps.i, taps.j, r, 3.0);
    EXPECT(points.taps() == 0);
    climate::ObsTaps bad = taps;
    bad.di[0] = 6;  // beyond lx = 5 of loc 3
    EXPECT(throws([&] { e.obs_network(bad, r, 3.0); }));

    // h of a member: every product rounded, summed from +0 in tap order (volatile keeps the compiler from contracting)
    auto h = [&](const std::vector<double>& f, std::size_t member, std::size_t o) {
        volatile double acc = 0.0;
        for (int s = taps.start[o]; s < taps.start[o + 1]; ++s) {
            volatile double p = taps.w[s] * f[member * cells + (taps.j[o] + taps.dj[s]) * (nx + 2) + taps.i[o] + taps.di[s]];
            acc = acc + p;
        }
        return static_cast<double>(acc);
    };
    net.observe(t, 11, 0, false);
    e.assimilate(net, 1.0, t, true);
    const climate::ObsValues v = net.fetch(true, true);
    const std::vector<double> A = e.download_all();
    EXPECT(A != X);
    for (std::size_t o = 0; o < 6; ++o) {
        EXPECT(v.truth[o] == h(X, t, o) && v.y[o] == v.truth[o]);
        // mv of h over the forecast members before and after the analysis
        for (int pass = 0; pass < 2; ++pass) {
            const std::vector<double>& f = pass ? A : X;
            volatile double s = 0.0;
            for (int k = 0; k < B; ++k)
                if (k != t) s = s + h(f, k, o);
            const double m = s / (B - 1);
            EXPECT((pass ? v.post_mean[o] : v.bg_mean[o]) == m);
        }
        EXPECT(v.bg_var[o] > 0.0 && v.post_var[o] > 0.0);
    }
    for (std::size_t c = 0; c < cells; ++c) EXPECT(A[t * cells + c] == X[t * cells + c]);  // the truth member
    const std::vector<csim_obs_cycle> log = net.log();
    EXPECT(log.size() == 1 && log[0].n == 6.0 && log[0].has_truth == 1.0);
    EXPECT(log[0].sum_r == ((((0.5 + 0.25) + 1.0) + 0.1) + 0.7) + 0.3);
    EXPECT(std::isfinite(log[0].sum_ea2) && log[0].sum_eb2 > 0.0);
    std::printf("obsop ok\n");
    return 0;
}
