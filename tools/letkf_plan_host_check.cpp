// tools/letkf_plan_host_check.cpp — the host side of the LETKF (csrc/assim_plan.cpp, csrc/assim_plan.hpp,
// csrc/letkf_nodes.hpp: the per-node lookup letkf_lookup_build, csim_letkf_nodes, csim_letkf_blend, csim_letkf_plan)
// under AddressSanitizer and UndefinedBehaviorSanitizer (tools/obsop_sanitize.sh).  A stand-alone program: no device, no
// HIP, nothing loaded into another process.  The lookup is compared node by node with brute force written here; the
// nodes and the blend are checked at their seams: nx, ny in {1, 2, 5, 13, 14} and spacings {1, 2, 4, 13, 100}, with
// observations on corners and edges, duplicate cells and half-widths larger than the grid.  Prints "letkf plan host
// ok" and returns 0, or says what failed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "assim_plan.hpp"
#include "letkf_nodes.hpp"

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
using csim::LetkfLookup;

// a plan whose order is not the input order: by (i + j) parity first, as two levels would put it
AssimPlan plan_of(const std::vector<int>& i, const std::vector<int>& j, int lx, int ly) {
    AssimPlan p;
    p.nobs = static_cast<int>(i.size()), p.lx = lx, p.ly = ly;
    for (int par = 0; par < 2; ++par)
        for (int o = 0; o < p.nobs; ++o)
            if (((i[o] + j[o]) & 1) == par) p.idx.push_back(o), p.pi.push_back(i[o]), p.pj.push_back(j[o]);
    return p;
}

int check_nodes(int nx, int ny, int s) {
    int nax = -1, nay = -1;
    EXPECT(csim_letkf_nodes(nx, ny, s, &nax, &nay, nullptr, nullptr) == CSIM_OK);
    EXPECT(nax == (nx == 1 ? 1 : (nx - 1 + s - 1) / s + 1) && nay == (ny == 1 ? 1 : (ny - 1 + s - 1) / s + 1));
    // heap arrays of exactly the sizes the call may touch
    std::vector<int> xi(nax, -1), yj(nay, -1);
    EXPECT(csim_letkf_nodes(nx, ny, s, nullptr, nullptr, xi.data(), yj.data()) == CSIM_OK);
    EXPECT(xi.front() == 1 && xi.back() == nx && yj.front() == 1 && yj.back() == ny);
    for (int a = 0; a + 1 < nax; ++a) EXPECT(xi[a] == 1 + a * s && xi[a + 1] > xi[a] && xi[a + 1] - xi[a] <= s);
    for (int b = 0; b + 1 < nay; ++b) EXPECT(yj[b] == 1 + b * s && yj[b + 1] > yj[b] && yj[b + 1] - yj[b] <= s);
    long nodes = -1;
    long long bytes = -1;
    EXPECT(csim_letkf_plan(5, nx, ny, s, &nodes, &bytes) == CSIM_OK && nodes == static_cast<long>(nax) * nay);
    EXPECT(bytes >= static_cast<long long>(nodes) * 8 * (36 + 2 * 25 + 2 * 5 + 1));
    for (int j = 1; j <= ny; ++j)
        for (int i = 1; i <= nx; ++i) {
            int node[4] = {-1, -1, -1, -1};
            double beta[4] = {-1, -1, -1, -1};
            EXPECT(csim_letkf_blend(nx, ny, s, i, j, node, beta) == CSIM_OK);
            double sum = 0.0, px = 0.0, py = 0.0;
            for (int n = 0; n < 4; ++n) {
                EXPECT(node[n] >= 0 && node[n] < nax * nay && beta[n] >= 0.0 && beta[n] <= 1.0);
                sum += beta[n], px += beta[n] * xi[node[n] % nax], py += beta[n] * yj[node[n] / nax];
            }
            // the weights sum to 1 and reproduce the cell's own position from the nodes' positions
            EXPECT(std::fabs(sum - 1.0) <= 4e-16 && std::fabs(px - i) <= 1e-12 * nx && std::fabs(py - j) <= 1e-12 * ny);
            // the interval holds the cell
            EXPECT(xi[node[0] % nax] <= i && i <= xi[node[3] % nax] && yj[node[0] / nax] <= j && j <= yj[node[3] / nax]);
            const bool on = std::find(xi.begin(), xi.end(), i) != xi.end() && std::find(yj.begin(), yj.end(), j) != yj.end();
            if (on) {
                int ones = 0;
                for (int n = 0; n < 4; ++n) {
                    EXPECT(beta[n] == 0.0 || beta[n] == 1.0);
                    if (beta[n] == 1.0) {
                        ++ones;
                        EXPECT(xi[node[n] % nax] == i && yj[node[n] / nax] == j);
                    }
                }
                EXPECT(ones == 1);
            }
        }
    return 0;
}

int check_lookup(int nx, int ny, int s, int lx, int ly, const std::vector<int>& i, const std::vector<int>& j) {
    const AssimPlan p = plan_of(i, j, lx, ly);
    LetkfLookup lk;
    EXPECT(csim::letkf_lookup_build(nx, ny, p, s, &lk));
    const int nax = csim::letkf_axis_nodes(nx, s), nay = csim::letkf_axis_nodes(ny, s);
    EXPECT(lk.spacing == s && lk.nax == nax && lk.nay == nay);
    EXPECT(lk.start.size() == static_cast<size_t>(nax) * nay + 1 && lk.start.front() == 0);
    EXPECT(static_cast<size_t>(lk.start.back()) == lk.pos.size());
    for (int b = 0; b < nay; ++b)
        for (int a = 0; a < nax; ++a) {
            const int ci = csim::letkf_node_at(a, s, nx), cj = csim::letkf_node_at(b, s, ny);
            std::vector<int> want;  // plan positions by increasing input index
            for (int o = 0; o < p.nobs; ++o)
                if (std::abs(ci - i[o]) <= lx && std::abs(cj - j[o]) <= ly)
                    want.push_back(static_cast<int>(std::find(p.idx.begin(), p.idx.end(), o) - p.idx.begin()));
            const size_t g = static_cast<size_t>(b) * nax + a;
            const std::vector<int> got(lk.pos.begin() + lk.start[g], lk.pos.begin() + lk.start[g + 1]);
            EXPECT(got == want);
        }
    return 0;
}

}  // namespace

int main() {
    const int sizes[] = {1, 2, 5, 13, 14}, spacings[] = {1, 2, 4, 13, 100};
    for (int nx : sizes)
        for (int ny : sizes)
            for (int s : spacings) {
                if (check_nodes(nx, ny, s)) return 1;
                // corners, an edge, a duplicate, the middle
                std::vector<int> i = {1, nx, 1, nx, (nx + 1) / 2, (nx + 1) / 2, std::min(2, nx)};
                std::vector<int> j = {1, ny, ny, 1, (ny + 1) / 2, (ny + 1) / 2, std::min(3, ny)};
                for (int l : {0, 1, 4, 40})
                    if (check_lookup(nx, ny, s, l, std::max(0, l - 1), i, j)) return 1;
            }
    // a larger grid with scattered observations
    {
        std::vector<int> i, j;
        unsigned v = 12345u;
        for (int o = 0; o < 200; ++o) {
            v = v * 1664525u + 1013904223u;
            i.push_back(1 + static_cast<int>((v >> 8) % 61));
            v = v * 1664525u + 1013904223u;
            j.push_back(1 + static_cast<int>((v >> 8) % 37));
        }
        for (int s : {1, 3, 8, 16})
            if (check_lookup(61, 37, s, 5, 3, i, j)) return 1;
    }
    // without observations every list is empty
    if (check_lookup(13, 9, 4, 2, 2, {}, {})) return 1;
    // errors
    int node[4];
    double beta[4];
    EXPECT(csim_letkf_nodes(0, 5, 1, nullptr, nullptr, nullptr, nullptr) == CSIM_ERR_ARG);
    EXPECT(csim_letkf_nodes(5, 5, 0, nullptr, nullptr, nullptr, nullptr) == CSIM_ERR_ARG);
    EXPECT(csim_letkf_blend(5, 5, 2, 6, 1, node, beta) == CSIM_ERR_ARG);
    EXPECT(csim_letkf_blend(5, 5, 2, 1, 1, nullptr, beta) == CSIM_ERR_ARG);
    EXPECT(csim_letkf_plan(1, 5, 5, 2, nullptr, nullptr) == CSIM_ERR_ARG);
    EXPECT(csim_letkf_plan(CSIM_ESPACE_MAX_MEMBERS + 1, 5, 5, 2, nullptr, nullptr) == CSIM_ERR_UNSUPPORTED);
    // the largest spacing and grid an int holds
    int nax = 0, nay = 0;
    EXPECT(csim_letkf_nodes(2147483647, 2, 2147483647, &nax, &nay, nullptr, nullptr) == CSIM_OK && nax == 2 && nay == 2);
    EXPECT(csim_letkf_nodes(2147483647, 1, 1, &nax, &nay, nullptr, nullptr) == CSIM_OK && nax == 2147483647 && nay == 1);
    std::printf("letkf plan host ok\n");
    return 0;
}
