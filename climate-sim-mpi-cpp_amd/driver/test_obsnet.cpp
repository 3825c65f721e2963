// test_obsnet.cpp — climate::ObsNetwork (include/climate/ensemble.hpp) on a GPU: the analysis through a network gives
// the bits of Ensemble::assimilate, the log and the diagnostics come back, and a network may outlive its ensemble.
// Prints "obsnet ok" and returns 0, or says what failed and returns 1.
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

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0;
}

template <class F> static bool throws(F&& f) {
    try {
        f();
    } catch (const std::exception&) {
        return true;
    }
    return false;
}

int main() {
    const int B = 6, nx = 40, ny = 24, bc[4] = {0, 1, 2, 0};
    std::mt19937_64 gen(7);
    std::normal_distribution<double> normal;
    std::vector<double> X(static_cast<std::size_t>(B) * (nx + 2) * (ny + 2));
    for (double& v : X) v = normal(gen);
    const std::vector<int> i = {1, 40, 20, 21, 7, 33}, j = {1, 24, 12, 13, 20, 5};
    const std::vector<double> r = {0.5, 0.25, 1.0, 0.1, 0.7, 0.3};

    auto a = std::make_unique<climate::Ensemble>(B, nx, ny, 1.0, 1.0, bc);
    climate::Ensemble b(B, nx, ny, 1.0, 1.0, bc);
    a->upload_all(X), b.upload_all(X);
    climate::ObsNetwork net = a->obs_network(i, j, r, 3.0, false, 2);
    EXPECT(net.size() == 6 && net.levels() >= 2);
    EXPECT(throws([&] { a->assimilate(net); }));  // no values yet
    net.observe(2, 11, 0);
    a->assimilate(net, 1.05, 2, true);
    const climate::ObsValues v = net.fetch(true, true);
    const climate::EnsembleAnalysis an = b.assimilate(i, j, v.y, r, 3.0, 1.05, 2);
    EXPECT(same_bits(a->download_all(), b.download_all()));
    EXPECT(!same_bits(a->download_all(), X));
    EXPECT(same_bits(v.post_mean, an.post_mean) && same_bits(v.post_var, an.post_var));
    const std::vector<double> truth = b.download(2);
    for (std::size_t o = 0; o < i.size(); ++o)
        EXPECT(v.truth[o] == X[2 * static_cast<std::size_t>((nx + 2) * (ny + 2)) + j[o] * (nx + 2) + i[o]] &&
               v.truth[o] == truth[j[o] * (nx + 2) + i[o]]);
    const std::vector<csim_obs_cycle> log = net.log();
    EXPECT(log.size() == 1 && log[0].n == 6.0 && log[0].has_truth == 1.0 && log[0].sum_va <= log[0].sum_vb);
    EXPECT(log[0].sum_r == ((((0.5 + 0.25) + 1.0) + 0.1) + 0.7) + 0.3);
    EXPECT(throws([&] { b.assimilate(net); }));  // a network of another ensemble

    // moves; a network destroyed before its ensemble; networks that outlive it
    climate::ObsNetwork moved = std::move(net);
    EXPECT(moved.log().size() == 1);
    {
        climate::ObsNetwork early = a->obs_network(i, j, r, 3.0);
        early.set_values(v.y);
    }
    climate::ObsNetwork late = a->obs_network(i, j, r, 3.0);
    late = a->obs_network(i, j, r, 2.0);  // move assignment destroys the one held
    a.reset();
    EXPECT(throws([&] { moved.log(); }) && throws([&] { late.set_values(v.y); }));
    EXPECT(throws([&] { b.assimilate(moved); }));
    late = std::move(moved);
    std::printf("obsnet ok\n");
    return 0;
}
