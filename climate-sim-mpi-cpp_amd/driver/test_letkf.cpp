// test_letkf.cpp — the LETKF through climate::Ensemble (include/climate/ensemble.hpp) on a GPU: Ensemble::assimilate_letkf
// and letkf_info against the C entry points on a twin (the same bits), climate::letkf_nodes and letkf_blend against the
// C calls, on one 37 x 21 case of 12 forecast members with 40 bilinear observations, two of them masked, at spacing 4
// and, on a second pair, at spacing 1 recorded; and what is refused.  Prints "letkf ok" and returns 0, or says what
// failed and returns 1.
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
    const std::size_t cells = static_cast<std::size_t>(nx + 2) * (ny + 2);
    std::mt19937_64 gen(12);
    std::normal_distribution<double> normal;
    std::uniform_real_distribution<double> px(1.0, nx), py(1.0, ny), pr(0.5, 2.0);
    std::vector<double> X(static_cast<std::size_t>(B) * cells), x(nobs), y(nobs), r(nobs), vals(nobs);
    for (double& v : X) v = 2.0 + normal(gen);
    for (int o = 0; o < nobs; ++o) x[o] = px(gen), y[o] = py(gen), r[o] = pr(gen), vals[o] = 2.0 + normal(gen);
    std::vector<unsigned char> mask(nobs, 1);
    mask[3] = mask[17] = 0;

    // the host-only calls
    for (int s : {1, 4, 100}) {
        const climate::LetkfNodes n = climate::letkf_nodes(nx, ny, s);
        int nax = 0, nay = 0;
        EXPECT(csim_letkf_nodes(nx, ny, s, &nax, &nay, nullptr, nullptr) == CSIM_OK && nax == n.nax && nay == n.nay);
        EXPECT(n.xi.front() == 1 && n.xi.back() == nx && n.yj.front() == 1 && n.yj.back() == ny);
        long nodes = 0;
        long long bytes = 0;
        EXPECT(csim_letkf_plan(M, nx, ny, s, &nodes, &bytes) == CSIM_OK && nodes == static_cast<long>(nax) * nay && bytes > 0);
        const climate::LetkfBlend b = climate::letkf_blend(nx, ny, s, 6, 3);
        int node[4];
        double beta[4];
        EXPECT(csim_letkf_blend(nx, ny, s, 6, 3, node, beta) == CSIM_OK);
        EXPECT(std::memcmp(node, b.node, sizeof node) == 0 && std::memcmp(beta, b.beta, sizeof beta) == 0);
        EXPECT(beta[0] + beta[1] + beta[2] + beta[3] > 0.999999 && beta[0] + beta[1] + beta[2] + beta[3] < 1.000001);
    }
    EXPECT(throws([&] { climate::letkf_nodes(nx, ny, 0); }));
    EXPECT(throws([&] { climate::letkf_blend(nx, ny, 4, nx + 1, 1); }));

    const climate::ObsTaps taps = climate::Ensemble::bilinear_taps(nx, ny, x, y);
    for (int s : {4, 1}) {
        const bool record = s == 1;
        climate::Ensemble a(B, nx, ny, 1.0, 1.0, bc);
        a.upload_all(X);
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
        EXPECT(throws([&] { a.letkf_info(); }));  // no analysis yet

        a.assimilate_letkf(na, inflation, t, record, 0.0, s);
        EXPECT(csim_ensemble_assimilate_letkf(eb, nb, inflation, t, record ? 1 : 0, 0.0, s) == CSIM_OK);
        const climate::LetkfInfo r1 = a.letkf_info();
        const climate::LetkfNodes n = climate::letkf_nodes(nx, ny, s);
        const std::size_t nn = static_cast<std::size_t>(n.nax) * n.nay;
        EXPECT(r1.nax == n.nax && r1.nay == n.nay && r1.dfs.size() == nn && r1.status.size() == nn);
        int nax = 0, nay = 0;
        std::vector<double> dfs(nn);
        std::vector<int> count(nn), sweeps(nn), status(nn);
        EXPECT(csim_ensemble_letkf_info(eb, &nax, &nay, dfs.data(), count.data(), sweeps.data(), status.data()) == CSIM_OK);
        EXPECT(nax == n.nax && nay == n.nay && same_bits(dfs, r1.dfs) && count == r1.count && sweeps == r1.sweeps &&
               status == r1.status);
        int ok = 0, most = 0;
        for (std::size_t g = 0; g < nn; ++g) {
            EXPECT(status[g] == CSIM_LETKF_OK || status[g] == CSIM_LETKF_IDLE);
            EXPECT((status[g] == CSIM_LETKF_IDLE) == (count[g] == 0) && (count[g] > 0) == (dfs[g] > 0.0));
            ok += status[g] == CSIM_LETKF_OK, most = count[g] > most ? count[g] : most;
        }
        EXPECT(ok > 0 && most > 1 && most <= nobs - 2);
        std::vector<double> Xa = a.download_all(), Xb(X.size());
        EXPECT(csim_ensemble_download_all(eb, Xb.data()) == CSIM_OK);
        EXPECT(same_bits(Xa, Xb) && !same_bits(Xa, X));
        EXPECT(std::memcmp(&Xa[t * cells], &X[t * cells], sizeof(double) * cells) == 0);
        EXPECT(na.log().size() == (record ? 1u : 0u));
        if (record) EXPECT(na.screen_log().size() == 1 && na.screen_log()[0].n_inactive == 2.0);
        EXPECT(throws([&] { a.etkf_info(t); }));  // an LETKF is no ETKF analysis

        // refused, and nothing moves
        climate::Ensemble other(B, nx, ny, 1.0, 1.0, bc);
        EXPECT(throws([&] { other.assimilate_letkf(na, 1.0, t); }));              // another ensemble's network
        EXPECT(throws([&] { a.assimilate_letkf(na, 0.5, t); }));                  // inflation < 1
        EXPECT(throws([&] { a.assimilate_letkf(na, 1.0, t, false, 0.0, 0); }));   // spacing < 1
        EXPECT(csim_ensemble_assimilate_letkf(eb, nb, 1.0, t, 0, 0.0, 0) == CSIM_ERR_ARG);
        EXPECT(same_bits(a.download_all(), Xa));
        EXPECT(csim_ensemble_destroy(eb) == CSIM_OK);
    }
    std::printf("letkf ok\n");
    return 0;
}
