// tools/obsop_host_check.cpp — the host-only code of the linear observations under AddressSanitizer and
// UndefinedBehaviorSanitizer (tools/obsop_sanitize.sh): the two tap builders, csim_obs_linear_check and the layout
// arithmetic of a network's device buffer with its tap arrays (csrc/obs_taps.cpp, csrc/obs_taps.hpp).  A stand-alone
// program: no device, no HIP, nothing loaded into another process.  Output arrays are heap blocks of exactly the
// documented size, so a write past them is caught.  Prints "obsop host ok" and returns 0, or says what failed.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "obs_taps.hpp"

namespace csim {
static std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace csim

#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    using namespace csim;
    // ---- builders
    {
        std::vector<int> di(4), dj(4);
        std::vector<double> w(4);
        int i = 0, j = 0;
        const double xs[] = {1.0, 40.0, 12.3, 39.999999999, 1.0000000000000002};
        for (double x : xs)
            for (double y : {1.0, 28.0, 7.5}) {
                EXPECT(csim_obs_taps_bilinear(40, 28, x, y, &i, &j, di.data(), dj.data(), w.data()) == CSIM_OK);
                EXPECT(i >= 1 && i <= 39 && j >= 1 && j <= 27);
                for (int s = 0; s < 4; ++s) EXPECT(i + di[s] >= 1 && i + di[s] <= 40 && j + dj[s] >= 1 && j + dj[s] <= 28);
            }
        EXPECT(csim_obs_taps_bilinear(1, 1, 1.0, 1.0, &i, &j, di.data(), dj.data(), w.data()) == CSIM_OK);
        EXPECT(i == 1 && j == 1 && di[1] == 0 && dj[2] == 0 && w[0] == 1.0);
        EXPECT(csim_obs_taps_bilinear(INT_MAX, INT_MAX, static_cast<double>(INT_MAX), 1.0, &i, &j, di.data(), dj.data(),
                                      w.data()) == CSIM_OK);
        EXPECT(i == INT_MAX - 1 && w[1] == 1.0);
        for (double bad : {0.5, 40.5, std::nan(""), std::numeric_limits<double>::infinity(), -1e300, 1e300})
            EXPECT(csim_obs_taps_bilinear(40, 28, bad, 2.0, &i, &j, di.data(), dj.data(), w.data()) == CSIM_ERR_ARG);
        EXPECT(csim_obs_taps_bilinear(40, 28, 2.0, 2.0, nullptr, &j, di.data(), dj.data(), w.data()) == CSIM_ERR_ARG);
    }
    {
        std::vector<int> di(CSIM_OBS_MAX_TAPS), dj(CSIM_OBS_MAX_TAPS);
        std::vector<double> w(CSIM_OBS_MAX_TAPS);
        int n = 0;
        EXPECT(csim_obs_taps_box(40, 28, 1, 1, 7, 7, &n, di.data(), dj.data(), w.data()) == CSIM_OK && n == 64);
        EXPECT(csim_obs_taps_box(40, 28, 20, 14, 3, 4, &n, di.data(), dj.data(), w.data()) == CSIM_OK && n == 63);
        EXPECT(csim_obs_taps_box(40, 28, 20, 14, 6, 2, &n, di.data(), dj.data(), w.data()) == CSIM_ERR_UNSUPPORTED);
        EXPECT(csim_obs_taps_box(40, 28, 20, 14, INT_MAX, INT_MAX, &n, di.data(), dj.data(), w.data()) == CSIM_ERR_UNSUPPORTED);
        EXPECT(csim_obs_taps_box(INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, &n, di.data(), dj.data(), w.data()) ==
               CSIM_ERR_UNSUPPORTED);
        EXPECT(csim_obs_taps_box(INT_MAX, INT_MAX, INT_MAX, INT_MAX, 3, 3, &n, di.data(), dj.data(), w.data()) == CSIM_OK &&
               n == 16 && di[0] == -3 && di[15] == 0);
        EXPECT(csim_obs_taps_box(40, 28, 1, 1, INT_MAX, 0, &n, di.data(), dj.data(), w.data()) == CSIM_OK && n == 40);
        EXPECT(csim_obs_taps_box(40, 28, 0, 1, 1, 1, &n, di.data(), dj.data(), w.data()) == CSIM_ERR_ARG);
        EXPECT(csim_obs_taps_box(40, 28, 1, 1, -1, 1, &n, di.data(), dj.data(), w.data()) == CSIM_ERR_ARG);
        EXPECT(csim_obs_taps_box(40, 28, 1, 1, 1, 1, nullptr, di.data(), dj.data(), w.data()) == CSIM_ERR_ARG);
    }
    // ---- the check: arrays of exactly start[nobs] taps
    {
        const std::vector<int> i = {12, 1, 40}, j = {5, 1, 28};
        std::vector<int> start = {0, 2, 6, 70}, di(70, 0), dj(70, 0);
        std::vector<double> w(70, 0.25);
        di[0] = 5, dj[1] = -3, di[3] = 2, dj[4] = 3;
        for (int s = 6; s < 70; ++s) di[s] = -(s % 6), dj[s] = -(s % 4);
        auto run = [&] {
            return csim_obs_linear_check(40, 28, 5, 3, 3, i.data(), j.data(), start.data(), di.data(), dj.data(), w.data());
        };
        EXPECT(run() == CSIM_OK);
        di[0] = 6;
        EXPECT(run() == CSIM_ERR_ARG);
        di[0] = INT_MAX;  // i + di does not wrap
        EXPECT(run() == CSIM_ERR_ARG);
        di[0] = INT_MIN;
        EXPECT(run() == CSIM_ERR_ARG);
        di[0] = 5, dj[2] = -1;
        EXPECT(run() == CSIM_ERR_ARG);  // (1, 0): the ghost ring
        dj[2] = 0, w[69] = std::nan("");
        EXPECT(run() == CSIM_ERR_ARG);
        w[69] = 0.25;
        // a start that is out of order is refused before any tap is read: these would index far outside the arrays
        for (std::vector<int> bad : {std::vector<int>{1, 2, 6, 70}, {0, 2, 1, 70}, {0, 0, 6, 70}, {0, 2, 6, 71 + 64},
                                     {0, INT_MAX, INT_MAX, INT_MAX}, {0, -5, 6, 70}, {0, 2, 6, INT_MIN}}) {
            start = bad;
            EXPECT(run() == CSIM_ERR_ARG);
        }
        start = {0, 2, 6, 70};
        EXPECT(run() == CSIM_OK);
        EXPECT(csim_obs_linear_check(40, 28, 5, 3, 0, i.data(), j.data(), start.data(), di.data(), dj.data(), w.data()) ==
               CSIM_ERR_ARG);
        EXPECT(csim_obs_linear_check(40, 28, 5, 3, 3, i.data(), j.data(), nullptr, di.data(), dj.data(), w.data()) ==
               CSIM_ERR_ARG);

        // ---- the layout and the plan-order copy: every array lies inside the buffer, 256-byte aligned, none overlaps
        for (size_t n : {size_t(1), size_t(3), size_t(257), size_t(1) << 20})
            for (size_t nt : {size_t(0), n, 64 * n}) {
                const size_t chunks = (n + 255) / 256;
                const ObsLayout l = obs_layout(n, nt, 63, 1024 * n, 11 * chunks, 13 * 4);
                const size_t at[] = {l.i, l.j, l.idx, l.pos, l.r, l.sr, l.rho, l.tstart, l.toff, l.tw, l.fixed,
                                     l.xt, l.scal, l.bg, l.post, l.part, l.hp, l.log, l.total};
                const size_t need[] = {4 * n, 4 * n, 4 * n, 4 * n, 8 * n, 8 * n, 8 * 63, nt ? 4 * (n + 1) : 0, 4 * nt, 8 * nt,
                                       8 * n, 8 * n, 24 * n, 16 * n, 16 * n, 88 * chunks, 8 * 1024 * n, 8 * 13 * 4};
                for (int k = 0; k < 18; ++k) EXPECT(at[k] % 256 == 0 && at[k] + need[k] <= at[k + 1]);
                EXPECT(l.y == l.fixed);
            }
        const ObsLayout l = obs_layout(3, 70, 63, 64, 11, 0);
        std::vector<char> h(l.fixed, 0);
        const std::vector<int> idx = {2, 0, 1};  // plan position -> input index
        obs_taps_plan_order(3, idx.data(), start.data(), di.data(), dj.data(), w.data(), 400,
                            reinterpret_cast<int*>(h.data() + l.tstart), reinterpret_cast<int*>(h.data() + l.toff),
                            reinterpret_cast<double*>(h.data() + l.tw));
        const int* ts = reinterpret_cast<const int*>(h.data() + l.tstart);
        const int* to = reinterpret_cast<const int*>(h.data() + l.toff);
        EXPECT(ts[0] == 0 && ts[1] == 64 && ts[2] == 66 && ts[3] == 70);
        EXPECT(to[0] == dj[6] * 400 + di[6] && to[64] == 5 && to[65] == -3 * 400 && to[69] == dj[5] * 400 + di[5]);
    }
    std::printf("obsop host ok\n");
    return 0;
}
