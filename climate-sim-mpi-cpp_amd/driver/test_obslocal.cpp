// test_obslocal.cpp — the local analysis through climate::ObsNetwork / climate::Ensemble (include/climate/ensemble.hpp)
// on a GPU: Ensemble::assimilate_local and ObsNetwork::local_info against the C entry points on a twin (the same bits),
// a lone observation against the serial analysis at its cell, a screened and recorded call, and what is refused.
// Prints "obslocal ok" and returns 0, or says what failed and returns 1.
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
    const int B = 6, nx = 40, ny = 24, bc[4] = {0, 1, 2, 0};
    std::mt19937_64 gen(11);
    std::normal_distribution<double> normal;
    std::vector<double> X(static_cast<std::size_t>(B) * (nx + 2) * (ny + 2));
    for (double& v : X) v = normal(gen);
    const std::vector<int> i = {1, 40, 20, 21, 7, 33, 12, 28, 20}, j = {1, 24, 12, 13, 20, 5, 8, 17, 12};
    const std::vector<double> r = {0.5, 0.25, 1.0, 0.1, 0.7, 0.3, 0.4, 0.6, 0.9};
    const std::size_t n = i.size();
    std::vector<double> y(n);
    for (double& v : y) v = normal(gen);

    // the C++ methods on one ensemble, the C entry points on its twin
    climate::Ensemble a(B, nx, ny, 1.0, 1.0, bc), b(B, nx, ny, 1.0, 1.0, bc);
    a.upload_all(X), b.upload_all(X);
    climate::ObsNetwork net = a.obs_network(i, j, r, 3.0, false, 2);
    net.set_values(y);
    EXPECT(throws([&] { net.status(); }));  // no analysis yet
    csim_ensemble* eb = nullptr;
    {
        // a twin through the C ABI alone
        EXPECT(csim_ensemble_create(B, nx, ny, 1, 1.0, 1.0, bc, 0.0, &eb) == CSIM_OK);
        EXPECT(csim_ensemble_upload_all(eb, X.data()) == CSIM_OK);
    }
    csim_obs_network* nb = nullptr;
    EXPECT(csim_obs_network_create(eb, static_cast<int>(n), i.data(), j.data(), r.data(), 3.0, 0, 2, &nb) == CSIM_OK);
    EXPECT(csim_obs_network_set_values(nb, y.data()) == CSIM_OK);
    int most_c = 0, most_host = 0;
    EXPECT(csim_obs_network_local_info(nb, &most_c) == CSIM_OK);
    int lx = 0, ly = 0;
    EXPECT(csim_obs_network_info(nb, nullptr, nullptr, &lx, &ly) == CSIM_OK);
    EXPECT(csim_obs_local_count(nx, ny, static_cast<int>(n), i.data(), j.data(), lx, ly, nullptr, &most_host) == CSIM_OK);
    EXPECT(net.local_info() == most_c && most_c == most_host && most_c >= 3);  // (20,12), (21,13) and (20,12) again

    a.assimilate_local(net, 1.05, 2, true, 0.0);
    EXPECT(csim_ensemble_assimilate_local(eb, nb, 1.05, 2, 1, 0.0) == CSIM_OK);
    std::vector<unsigned long long> sa = a.checksums(), sb(B);
    EXPECT(csim_ensemble_checksum(eb, sb.data()) == CSIM_OK);
    EXPECT(sa == sb);
    b.upload_all(X);
    EXPECT(sa != b.checksums() && sa[2] == b.checksums()[2]);  // the forecast members moved, the truth member did not
    for (unsigned char s : net.status()) EXPECT(s == CSIM_OBS_USED);
    EXPECT(net.log().size() == 1 && net.log()[0].n == 9.0 && net.screen_log()[0].n_used == 9.0);

    // a lone observation: at its cell the members of the serial analysis
    {
        climate::Ensemble c(B, nx, ny, 1.0, 1.0, bc), d(B, nx, ny, 1.0, 1.0, bc);
        c.upload_all(X), d.upload_all(X);
        const std::vector<int> oi = {17}, oj = {9};
        const std::vector<double> orr = {0.4}, oy = {0.8};
        climate::ObsNetwork one = c.obs_network(oi, oj, orr, 3.0), two = d.obs_network(oi, oj, orr, 3.0);
        one.set_values(oy), two.set_values(oy);
        c.assimilate_local(one, 1.0, 2);
        d.assimilate(two, 1.0, 2);
        const std::vector<double> C = c.download_all(), D = d.download_all();
        const std::size_t slab = static_cast<std::size_t>(nx + 2) * (ny + 2), cell = 9 * static_cast<std::size_t>(nx + 2) + 17;
        for (int m = 0; m < B; ++m) EXPECT(C[m * slab + cell] == D[m * slab + cell]);
        EXPECT(C[cell] != X[cell] && one.local_info() == 1);
    }

    // screened and recorded: a missing report and a gross error
    climate::ObsValues v = net.fetch(false, true);
    for (std::size_t o = 0; o < n; ++o) y[o] = v.post_mean[o] + 0.25 * std::sqrt(v.post_var[o] + r[o]);
    y[4] = v.post_mean[4] + 40.0 * std::sqrt(v.post_var[4] + r[4]);
    net.set_values(y);
    std::vector<unsigned char> active(n, 1);
    active[1] = 0;
    net.set_active(active);
    a.assimilate_local(net, 1.0, 2, true, 3.0);
    const std::vector<unsigned char> st = net.status();
    EXPECT(st[1] == CSIM_OBS_INACTIVE && st[4] == CSIM_OBS_REJECTED && st[0] == CSIM_OBS_USED);
    const std::vector<csim_obs_screen_cycle> slog = net.screen_log();
    EXPECT(slog.size() == 2 && slog[1].n_used == 7.0 && slog[1].n_inactive == 1.0 && slog[1].n_rejected == 1.0);
    net.impact_capture(2);  // the last analysis was a recorded one

    EXPECT(throws([&] { a.assimilate_local(net, 1.0, 2, true); }));   // the log is full
    EXPECT(throws([&] { a.assimilate_local(net, 0.5, 2); }));
    EXPECT(throws([&] { a.assimilate_local(net, 1.0, 2, false, -1.0); }));
    EXPECT(throws([&] { b.assimilate_local(net, 1.0, 2); }));         // a network of another ensemble
    EXPECT(net.status() == st);

    EXPECT(csim_obs_network_destroy(nb) == CSIM_OK && csim_ensemble_destroy(eb) == CSIM_OK);
    std::printf("obslocal ok\n");
    return 0;
}
