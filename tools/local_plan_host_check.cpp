// tools/local_plan_host_check.cpp — the host side of the local analysis (csrc/assim_plan.cpp, csrc/assim_plan.hpp:
// csim_obs_local_count and the per-tile lookup local_tiles_build) under AddressSanitizer and UndefinedBehaviorSanitizer
// (tools/obsop_sanitize.sh).  A stand-alone program: no device, no HIP, nothing loaded into another process.  Both are
// compared with brute force written here: the count cell by cell, the lookup tile by tile.  The cases hold
// observations on corners and edges, duplicate cells, half-widths larger than the grid, and tiles that do not divide
// nx and ny.  Prints "local plan host ok" and returns 0, or says what failed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "assim_plan.hpp"

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

namespace {

using csim::AssimPlan;
using csim::LocalTiles;

struct Case {
    int nx, ny;
    std::vector<int> i, j;
};

bool inside(int ci, int cj, int io, int jo, int lx, int ly) { return std::abs(ci - io) <= lx && std::abs(cj - jo) <= ly; }

int check_count(const Case& c, int lx, int ly) {
    const int n = static_cast<int>(c.i.size());
    // heap arrays of exactly the sizes the call may touch
    std::vector<int> count(static_cast<size_t>(c.nx) * c.ny, -1);
    int most = -1;
    EXPECT(csim_obs_local_count(c.nx, c.ny, n, c.i.data(), c.j.data(), lx, ly, count.data(), &most) == CSIM_OK);
    int want_most = 0;
    for (int cj = 1; cj <= c.ny; ++cj)
        for (int ci = 1; ci <= c.nx; ++ci) {
            int want = 0;
            for (int o = 0; o < n; ++o) want += inside(ci, cj, c.i[o], c.j[o], lx, ly);
            EXPECT(count[static_cast<size_t>(cj - 1) * c.nx + (ci - 1)] == want);
            want_most = std::max(want_most, want);
        }
    EXPECT(most == want_most);
    int again = -1;
    EXPECT(csim_obs_local_count(c.nx, c.ny, n, c.i.data(), c.j.data(), lx, ly, nullptr, &again) == CSIM_OK && again == most);
    EXPECT(csim_obs_local_count(c.nx, c.ny, n, c.i.data(), c.j.data(), lx, ly, count.data(), nullptr) == CSIM_OK);
    return 0;
}

// the lookup of a plan whose order is a permutation of the input: every tile's entries are plan positions, of the
// observations whose clipped rectangle meets the tile, in increasing input index
int check_tiles(const Case& c, int lx, int ly, int tile) {
    const int n = static_cast<int>(c.i.size());
    AssimPlan p;
    p.nobs = n, p.lx = lx, p.ly = ly;
    // plan order: the input reversed in pairs, so that positions and indices differ
    p.idx.resize(n), p.pi.resize(n), p.pj.resize(n);
    for (int q = 0; q < n; ++q) p.idx[q] = n - 1 - q;
    for (int q = 0; q < n; ++q) p.pi[q] = c.i[p.idx[q]], p.pj[q] = c.j[p.idx[q]];
    LocalTiles t;
    EXPECT(csim::local_tiles_build(c.nx, c.ny, p, tile, &t));
    const int ntx = (c.nx + tile - 1) / tile, nty = (c.ny + tile - 1) / tile;
    EXPECT(t.tile == tile && t.ntx == ntx && t.nty == nty);
    EXPECT(static_cast<int>(t.start.size()) == ntx * nty + 1 && t.start[0] == 0);
    EXPECT(static_cast<size_t>(t.start.back()) == t.pos.size());
    for (int ty = 0; ty < nty; ++ty)
        for (int tx = 0; tx < ntx; ++tx) {
            const int T = ty * ntx + tx;
            std::vector<int> want;  // input indices, ascending
            for (int o = 0; o < n; ++o) {
                bool meets = false;
                for (int cj = ty * tile + 1; cj <= std::min(c.ny, (ty + 1) * tile); ++cj)
                    for (int ci = tx * tile + 1; ci <= std::min(c.nx, (tx + 1) * tile); ++ci)
                        meets = meets || inside(ci, cj, c.i[o], c.j[o], lx, ly);
                if (meets) want.push_back(o);
            }
            EXPECT(t.start[T] <= t.start[T + 1]);
            EXPECT(static_cast<size_t>(t.start[T + 1] - t.start[T]) == want.size());
            for (size_t k = 0; k < want.size(); ++k) {
                const int q = t.pos[t.start[T] + k];
                EXPECT(q >= 0 && q < n && p.idx[q] == want[k]);
            }
        }
    return 0;
}

}  // namespace

int main() {
    const std::vector<Case> cases = {
        {8, 6, {}, {}},
        {8, 6, {3}, {2}},
        {8, 6, {1, 8, 1, 8}, {1, 6, 6, 1}},                                  // the corners
        {8, 6, {1, 8, 4, 5}, {3, 4, 1, 6}},                                  // the edges
        {8, 6, {4, 4, 4, 4, 2}, {3, 3, 3, 3, 5}},                            // one cell four times
        {37, 21, {1, 37, 19, 19, 20, 5, 33, 12, 12}, {1, 21, 11, 11, 12, 20, 2, 7, 7}},
        {1, 1, {1, 1}, {1, 1}},
        {1, 9, {1, 1, 1}, {1, 5, 9}},
        {17, 16, {16, 17, 1, 9, 9}, {16, 1, 16, 8, 9}},                      // 17 = 16 + 1: a tile of one column
    };
    for (const Case& c : cases)
        for (int lx : {0, 1, 4, 40})            // 40: larger than every grid here
            for (int ly : {0, 2, 40}) {
                if (check_count(c, lx, ly)) {
                    std::printf("  in the count of %zu observations on %d x %d, lx %d, ly %d\n", c.i.size(), c.nx, c.ny, lx, ly);
                    return 1;
                }
                for (int tile : {4, 8, 16})
                    if (check_tiles(c, lx, ly, tile)) {
                        std::printf("  in the lookup of %zu observations on %d x %d, lx %d, ly %d, tile %d\n", c.i.size(),
                                    c.nx, c.ny, lx, ly, tile);
                        return 1;
                    }
            }
    // the argument checks, each with its code
    {
        const int i[1] = {3}, j[1] = {2}, out_i[1] = {9}, out_j[1] = {0};
        int most = 0;
        EXPECT(csim_obs_local_count(0, 6, 1, i, j, 1, 1, nullptr, &most) == CSIM_ERR_ARG);
        EXPECT(csim_obs_local_count(8, 0, 1, i, j, 1, 1, nullptr, &most) == CSIM_ERR_ARG);
        EXPECT(csim_obs_local_count(8, 6, -1, i, j, 1, 1, nullptr, &most) == CSIM_ERR_ARG);
        EXPECT(csim_obs_local_count(8, 6, 1, nullptr, j, 1, 1, nullptr, &most) == CSIM_ERR_ARG);
        EXPECT(csim_obs_local_count(8, 6, 1, i, nullptr, 1, 1, nullptr, &most) == CSIM_ERR_ARG);
        EXPECT(csim_obs_local_count(8, 6, 1, i, j, -1, 1, nullptr, &most) == CSIM_ERR_ARG);
        EXPECT(csim_obs_local_count(8, 6, 1, i, j, 1, -1, nullptr, &most) == CSIM_ERR_ARG);
        EXPECT(csim_obs_local_count(8, 6, 1, out_i, j, 1, 1, nullptr, &most) == CSIM_ERR_ARG &&
               csim::g_err == "observation outside the interior");
        EXPECT(csim_obs_local_count(8, 6, 1, i, out_j, 1, 1, nullptr, &most) == CSIM_ERR_ARG);
        EXPECT(csim_obs_local_count(8, 6, 0, nullptr, nullptr, 1, 1, nullptr, &most) == CSIM_OK && most == 0);
        // half-widths at the top of int: no overflow on the way to the clipped rectangle
        EXPECT(csim_obs_local_count(8, 6, 1, i, j, 2147483647, 2147483647, nullptr, &most) == CSIM_OK && most == 1);
    }
    std::printf("local plan host ok\n");
    return 0;
}
