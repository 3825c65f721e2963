// obs_taps.cpp — linear observations on the host (include/csim.h): the check that csim_obs_network_create_linear runs
// before anything is enqueued, and the two tap builders.  No device, no HIP headers (obs_taps.hpp).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "obs_taps.hpp"

using namespace csim;

extern "C" {

int csim_obs_linear_check(int nx, int ny, int lx, int ly, int nobs, const int* i, const int* j, const int* start,
                          const int* di, const int* dj, const double* w) {
    OBS_REQUIRE(nx >= 1 && ny >= 1, "empty grid");
    OBS_REQUIRE(lx >= 0 && ly >= 0, "lx and ly must be >= 0");
    OBS_REQUIRE(nobs >= 1, "nobs must be >= 1");
    OBS_REQUIRE(i && j && start && di && dj && w, "null observation array");
    OBS_REQUIRE(start[0] == 0, "start[0] must be 0");
    // start first, so that no tap index below is out of the arrays' range
    for (int o = 0; o < nobs; ++o) {
        OBS_REQUIRE(start[o + 1] >= start[o], "start must be non-decreasing");
        const int nt = start[o + 1] - start[o];
        OBS_REQUIRE(nt >= 1, "an observation needs at least one tap");
        OBS_REQUIRE(nt <= CSIM_OBS_MAX_TAPS, "an observation has at most CSIM_OBS_MAX_TAPS taps");
    }
    for (int o = 0; o < nobs; ++o) {
        OBS_REQUIRE(i[o] >= 1 && i[o] <= nx && j[o] >= 1 && j[o] <= ny, "observation outside the interior");
        for (int s = start[o]; s < start[o + 1]; ++s) {
            // 64-bit: di + i cannot wrap
            const long long ci = static_cast<long long>(i[o]) + di[s], cj = static_cast<long long>(j[o]) + dj[s];
            OBS_REQUIRE(ci >= 1 && ci <= nx && cj >= 1 && cj <= ny, "tap outside the interior");
            OBS_REQUIRE(std::llabs(static_cast<long long>(di[s])) <= lx && std::llabs(static_cast<long long>(dj[s])) <= ly,
                        "tap beyond the localisation half-width of its anchor");
            OBS_REQUIRE(std::isfinite(w[s]), "tap weight must be finite");
        }
    }
    return CSIM_OK;
}

int csim_obs_taps_bilinear(int nx, int ny, double x, double y, int* i, int* j, int di[4], int dj[4], double w[4]) {
    OBS_REQUIRE(i && j && di && dj && w, "null argument");
    OBS_REQUIRE(nx >= 1 && ny >= 1, "empty grid");
    OBS_REQUIRE(x >= 1.0 && x <= static_cast<double>(nx) && y >= 1.0 && y <= static_cast<double>(ny),
                "position outside 1 .. nx, 1 .. ny");  // false for a NaN
    const int ia = std::max(std::min(static_cast<int>(std::floor(x)), nx - 1), 1);
    const int ja = std::max(std::min(static_cast<int>(std::floor(y)), ny - 1), 1);
    const double fx = x - static_cast<double>(ia), fy = y - static_cast<double>(ja);
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    const int ex = nx == 1 ? 0 : 1, ey = ny == 1 ? 0 : 1;
    *i = ia, *j = ja;
    di[0] = 0, dj[0] = 0, w[0] = gx * gy;
    di[1] = ex, dj[1] = 0, w[1] = fx * gy;
    di[2] = 0, dj[2] = ey, w[2] = gx * fy;
    di[3] = ex, dj[3] = ey, w[3] = fx * fy;
    return CSIM_OK;
}

int csim_obs_taps_box(int nx, int ny, int i, int j, int a, int b, int* ntaps, int* di, int* dj, double* w) {
    OBS_REQUIRE(ntaps && di && dj && w, "null argument");
    OBS_REQUIRE(nx >= 1 && ny >= 1, "empty grid");
    OBS_REQUIRE(i >= 1 && i <= nx && j >= 1 && j <= ny, "observation outside the interior");
    OBS_REQUIRE(a >= 0 && b >= 0, "a and b must be >= 0");
    // clipped to the interior; 64-bit, since i + a may pass INT_MAX
    const long long a0 = std::max<long long>(-a, 1LL - i), a1 = std::min<long long>(a, static_cast<long long>(nx) - i);
    const long long b0 = std::max<long long>(-b, 1LL - j), b1 = std::min<long long>(b, static_cast<long long>(ny) - j);
    const long long count = (a1 - a0 + 1) * (b1 - b0 + 1);
    if (a1 - a0 + 1 > CSIM_OBS_MAX_TAPS || b1 - b0 + 1 > CSIM_OBS_MAX_TAPS || count > CSIM_OBS_MAX_TAPS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_obs_taps_box: more than CSIM_OBS_MAX_TAPS taps");
    const double each = 1.0 / static_cast<double>(count);
    int n = 0;
    for (long long v = b0; v <= b1; ++v)
        for (long long u = a0; u <= a1; ++u, ++n) di[n] = static_cast<int>(u), dj[n] = static_cast<int>(v), w[n] = each;
    *ntaps = n;
    return CSIM_OK;
}

}  // extern "C"
