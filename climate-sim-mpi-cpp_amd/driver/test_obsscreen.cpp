// test_obsscreen.cpp — screening through climate::ObsNetwork / climate::Ensemble (include/climate/ensemble.hpp) on a
// GPU: set_active, status and screen_log, the defaulted assimilate overload against the unscreened bits, a screened
// cycle's statuses against csim_obs_screen_decide on the fetched diagnostics, and handles that outlive the ensemble.
// Prints "obsscreen ok" and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdio>
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

int main() {
    const int B = 6, nx = 40, ny = 24, bc[4] = {0, 1, 2, 0};
    std::mt19937_64 gen(7);
    std::normal_distribution<double> normal;
    std::vector<double> X(static_cast<std::size_t>(B) * (nx + 2) * (ny + 2));
    for (double& v : X) v = normal(gen);
    const std::vector<int> i = {1, 40, 20, 21, 7, 33, 12, 28}, j = {1, 24, 12, 13, 20, 5, 8, 17};
    const std::vector<double> r = {0.5, 0.25, 1.0, 0.1, 0.7, 0.3, 0.4, 0.6};
    const std::size_t n = i.size();

    auto a = std::make_unique<climate::Ensemble>(B, nx, ny, 1.0, 1.0, bc);
    climate::Ensemble b(B, nx, ny, 1.0, 1.0, bc), c(B, nx, ny, 1.0, 1.0, bc);
    a->upload_all(X), b.upload_all(X), c.upload_all(X);
    climate::ObsNetwork net = a->obs_network(i, j, r, 3.0, true, 3);
    climate::ObsNetwork plain = b.obs_network(i, j, r, 3.0, true, 3);
    EXPECT(throws([&] { net.status(); }));  // no analysis yet
    EXPECT(throws([&] { net.set_active(std::vector<unsigned char>(n - 1, 1)); }));
    EXPECT(throws([&] { net.set_active(std::vector<unsigned char>(n, 2)); }));

    // nothing screened: the defaulted overload, an all-ones mask and set_all_active give the bits of before
    std::vector<double> y(n);
    for (double& v : y) v = normal(gen);
    net.set_values(y), plain.set_values(y);
    net.set_active(std::vector<unsigned char>(n, 1));
    a->assimilate(net, 1.05, 2, true);
    b.assimilate(plain, 1.05, 2, true);
    EXPECT(a->checksums() == b.checksums());
    for (unsigned char s : net.status()) EXPECT(s == CSIM_OBS_USED);
    net.set_all_active();
    a->assimilate(net, 1.0, 2, true, 1e6);
    b.assimilate(plain, 1.0, 2, true);
    EXPECT(a->checksums() == b.checksums());
    std::vector<csim_obs_screen_cycle> slog = net.screen_log();
    EXPECT(slog.size() == 2 && slog[1].n_used == 8.0 && slog[1].n_inactive == 0.0 && slog[1].n_rejected == 0.0);
    EXPECT(net.log()[1].n == 8.0 && net.log()[1].sum_r == plain.log()[1].sum_r);

    // a screened cycle: two missing reports, two gross errors; statuses = csim_obs_screen_decide of the diagnostics
    const double tol = 3.0;
    climate::ObsValues v = net.fetch(false, true);  // post_* of the last analysis: the background of the next
    const std::vector<unsigned char> active = {1, 0, 1, 1, 1, 0, 1, 1};
    for (std::size_t o = 0; o < n; ++o) y[o] = v.post_mean[o] + 0.25 * std::sqrt(v.post_var[o] + r[o]);
    y[2] = v.post_mean[2] + 40.0 * std::sqrt(v.post_var[2] + r[2]);
    y[6] = v.post_mean[6] - 40.0 * std::sqrt(v.post_var[6] + r[6]);
    y[1] = 1e30;
    net.set_values(y);
    net.set_active(active);
    c.upload_all(a->download_all());
    a->assimilate(net, 1.0, 2, true, tol);
    const std::vector<unsigned char> st = net.status();
    v = net.fetch(false, true);
    int used = 0, inactive = 0, rejected = 0;
    std::vector<int> ui, uj;
    std::vector<double> uy, ur;
    for (std::size_t o = 0; o < n; ++o) {
        int want = -1;
        EXPECT(csim_obs_screen_decide(y[o], v.bg_mean[o], v.bg_var[o], r[o], tol, active[o], &want) == CSIM_OK);
        EXPECT(st[o] == want);
        used += want == CSIM_OBS_USED, inactive += want == CSIM_OBS_INACTIVE, rejected += want == CSIM_OBS_REJECTED;
        if (want == CSIM_OBS_USED) ui.push_back(i[o]), uj.push_back(j[o]), uy.push_back(y[o]), ur.push_back(r[o]);
    }
    EXPECT(used == 4 && inactive == 2 && rejected == 2 && st[2] == CSIM_OBS_REJECTED && st[1] == CSIM_OBS_INACTIVE);
    slog = net.screen_log();
    EXPECT(slog.size() == 3 && slog[2].n_used == 4.0 && slog[2].n_inactive == 2.0 && slog[2].n_rejected == 2.0);
    EXPECT(net.log()[2].n == 4.0 && net.log()[2].sum_r == ((0.5 + 0.1) + 0.7) + 0.6);
    // ordered: the analysis of the used observations alone
    c.assimilate_enqueue(ui, uj, uy, ur, 3.0, 1.0, 2, true);
    EXPECT(a->checksums() == c.checksums() && a->checksums() != b.checksums());
    EXPECT(throws([&] { a->assimilate(net, 1.0, 2, false, -1.0); }));
    EXPECT(throws([&] { a->assimilate(net, 1.0, 2, true, tol); }));  // the log is full
    EXPECT(throws([&] { b.assimilate(net, 1.0, 2, false, tol); }));  // a network of another ensemble
    EXPECT(net.status() == st);

    // a network that outlives its ensemble: every call throws, destroying and moving it is safe
    climate::ObsNetwork moved = std::move(net);
    EXPECT(moved.status() == st && moved.screen_log().size() == 3);
    a.reset();
    EXPECT(throws([&] { moved.status(); }) && throws([&] { moved.screen_log(); }));
    EXPECT(throws([&] { moved.set_active(active); }) && throws([&] { moved.set_all_active(); }));
    EXPECT(throws([&] { b.assimilate(moved, 1.0, 2, false, tol); }));
    plain = std::move(moved);
    std::printf("obsscreen ok\n");
    return 0;
}
