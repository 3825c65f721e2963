// test_held.cpp — one window of the 4D-ETKF through climate::ObsNetwork and climate::Ensemble
// (include/climate/ensemble.hpp) on a GPU: set_slots, then for every slot in increasing order hold and run, then
// assimilate_etkf_held on the path the case names.  The case comes from a file and the members and the transformed rows
// go to another, so that tests/test_gpu_held_cpp.py can hold them against the Python path bit for bit.
//   test_held <case> <out>
//   case: int32 B, t, nx, ny, nobs, steps, device, bc[4]; double inflation, D, dt, vx, vy, loc, bc_value;
//         int32 i[nobs], j[nobs], slot[nobs]; double r[nobs], y[nobs], X[B (nx+2)(ny+2)]
//   out:  double members[B (nx+2)(ny+2)], rows[nobs M]
// Prints "held ok" and returns 0, or says what failed and returns 1.
#include <algorithm>
#include <cstdio>
#include <set>

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

template <class T> static bool read_n(std::FILE* f, std::vector<T>& v, std::size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    EXPECT(argc == 3);
    std::FILE* in = std::fopen(argv[1], "rb");
    EXPECT(in);
    std::vector<int> head, i, j, slot;
    std::vector<double> par, r, y, X;
    EXPECT(read_n(in, head, 11) && read_n(in, par, 7));
    const int B = head[0], t = head[1], nx = head[2], ny = head[3], nobs = head[4], steps = head[5];
    const bool device = head[6] != 0;
    const int bc[4] = {head[7], head[8], head[9], head[10]};
    EXPECT(B >= 2 && nx >= 1 && ny >= 1 && nobs >= 1 && steps >= 0);
    const std::size_t cells = static_cast<std::size_t>(nx + 2) * (ny + 2), M = static_cast<std::size_t>(t >= 0 ? B - 1 : B);
    EXPECT(read_n(in, i, nobs) && read_n(in, j, nobs) && read_n(in, slot, nobs));
    EXPECT(read_n(in, r, nobs) && read_n(in, y, nobs) && read_n(in, X, B * cells));
    std::fclose(in);

    climate::Ensemble e(B, nx, ny, 1.0, 1.0, bc, par[6]);
    e.upload_all(X);
    auto all = [&](double v) { return std::vector<double>(B, v); };
    e.set_physics(all(par[1]), all(par[2]), all(par[3]), all(par[4]));
    climate::ObsNetwork net = e.obs_network(i, j, r, par[5], false, 1);
    net.set_values(y);
    net.set_slots(slot);
    EXPECT(throws([&] { net.held(); }));                                       // nothing held yet
    EXPECT(throws([&] { e.assimilate_etkf_held(net, par[0], t, false, 0.0, device); }));
    for (int s : std::set<int>(slot.begin(), slot.end())) {
        net.hold(s, t);
        e.run(steps);
    }
    const std::vector<double> H = net.held();
    EXPECT(H.size() == nobs * M);
    const climate::ObsGram g = e.obs_gram_held(net, true);
    EXPECT(g.A.size() == (M + 1) * (M + 1) && g.loglik.size() == M && g.n_used == nobs);
    e.assimilate_etkf_held(net, par[0], t, true, 0.0, device);
    const climate::EtkfAnalysis info = e.etkf_info(t);
    EXPECT(info.n_used == nobs && info.chi2 == g.A.back());
    const std::vector<double> Xa = e.download_all(), Ha = net.held();
    EXPECT(Xa != X && Ha != H && Ha.size() == H.size());
    EXPECT(net.log().size() == 1);
    EXPECT(throws([&] { e.assimilate_etkf_held(net, par[0], t, false, 0.0, device); }));   // the window is over
    EXPECT(throws([&] { net.impact_capture(t); }));                                         // not built for held rows
    EXPECT(throws([&] { net.set_slots(std::vector<int>(nobs, 64)); }));
    EXPECT(e.download_all() == Xa);

    std::FILE* out = std::fopen(argv[2], "wb");
    EXPECT(out);
    EXPECT(std::fwrite(Xa.data(), sizeof(double), Xa.size(), out) == Xa.size());
    EXPECT(std::fwrite(Ha.data(), sizeof(double), Ha.size(), out) == Ha.size());
    EXPECT(std::fclose(out) == 0);
    std::printf("held ok\n");
    return 0;
}
