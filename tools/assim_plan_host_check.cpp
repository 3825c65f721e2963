// tools/assim_plan_host_check.cpp — the analysis plan (csrc/assim_plan.cpp, csrc/assim_plan.hpp) and the byte layout
// of the one-shot analysis (csrc/obs_taps.hpp) under AddressSanitizer and UndefinedBehaviorSanitizer
// (tools/obsop_sanitize.sh).  A stand-alone program: no device, no HIP, nothing loaded into another process.  Levels
// are compared with brute-force assignments written here, the plan order and the batches with their definitions, and
// every per-observation fault with its code and text.  Prints "assim plan host ok" and returns 0, or says what failed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
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

using csim::AssimBatch;
using csim::AssimPlan;

constexpr int NX = 8, NY = 6;

bool conflict(int ia, int ja, int ib, int jb, int lx, int ly) {
    return std::abs(ia - ib) <= 2 * lx && std::abs(ja - jb) <= 2 * ly;
}

// first fit: the lowest level none of whose observations conflicts; ordered: one above every earlier conflict
std::vector<int> brute_levels(const std::vector<int>& i, const std::vector<int>& j, int lx, int ly, bool ordered) {
    const int n = static_cast<int>(i.size());
    std::vector<int> lev(n);
    for (int o = 0; o < n; ++o) {
        int lv = 0;
        if (ordered) {
            for (int p = 0; p < o; ++p)
                if (conflict(i[p], j[p], i[o], j[o], lx, ly)) lv = std::max(lv, lev[p] + 1);
        } else {
            for (;; ++lv) {
                bool hit = false;
                for (int p = 0; p < o; ++p) hit = hit || (lev[p] == lv && conflict(i[p], j[p], i[o], j[o], lx, ly));
                if (!hit) break;
            }
        }
        lev[o] = lv;
    }
    return lev;
}

// heap arrays of exactly n values, so that a read or write past them is caught
struct Case {
    std::vector<int> i, j;
};

// levels, plan order and batches of one case under half-widths that `loc` gives on the NX x NY grid of unit spacing
int check_case(const Case& c, double loc, bool ordered) {
    const int n = static_cast<int>(c.i.size());
    int lx = 0, ly = 0;
    EXPECT(csim_ensemble_gc_table(1.0, 1.0, loc, NX, NY, &lx, &ly, nullptr) == CSIM_OK);
    const std::vector<int> want = brute_levels(c.i, c.j, lx, ly, ordered);
    const int want_nl = n ? *std::max_element(want.begin(), want.end()) + 1 : 0;

    std::vector<int> lev(n);
    int nl = -1;
    EXPECT(csim_ensemble_assim_plan(n, c.i.data(), c.j.data(), lx, ly, ordered, lev.data(), &nl) == CSIM_OK);
    EXPECT(nl == want_nl && lev == want);

    const std::vector<double> r(n, 0.5), y(n, 1.0);
    AssimPlan p;
    EXPECT(csim::assim_plan_build(NX, NY, 1.0, 1.0, loc, ordered, n, c.i.data(), c.j.data(), r.data(), y.data(), &p) ==
           CSIM_OK);
    EXPECT(p.nobs == n && p.nlevels == want_nl && p.lx == lx && p.ly == ly);
    EXPECT(static_cast<int>(p.off.size()) == want_nl + 1 && static_cast<int>(p.idx.size()) == n);
    EXPECT(static_cast<int>(p.pi.size()) == n && static_cast<int>(p.pj.size()) == n);
    EXPECT(p.off[0] == 0 && p.off[want_nl] == n);
    std::vector<int> seen(n, 0);
    for (int L = 0; L < want_nl; ++L) {
        EXPECT(p.off[L] <= p.off[L + 1]);
        for (int q = p.off[L]; q < p.off[L + 1]; ++q) {
            const int o = p.idx[q];
            EXPECT(o >= 0 && o < n);
            ++seen[o];
            EXPECT(want[o] == L);
            EXPECT(q == p.off[L] || p.idx[q - 1] < o);
            EXPECT(p.pi[q] == c.i[o] && p.pj[q] == c.j[o]);
        }
    }
    for (int o = 0; o < n; ++o) EXPECT(seen[o] == 1);

    for (int batch : {1, 2, n + 3}) {
        std::vector<AssimBatch> b;
        csim::assim_batches(NX, NY, p, batch, &b);
        std::vector<int> in(n, 0);
        for (const AssimBatch& k : b) {
            EXPECT(k.count >= 1 && k.count <= batch && k.first >= 0 && k.first + k.count <= n);
            int L = 0;
            while (p.off[L + 1] <= k.first) ++L;
            EXPECT(k.first + k.count <= p.off[L + 1]);  // within one level
            long w = 0;
            for (int q = k.first; q < k.first + k.count; ++q) {
                ++in[q];
                long cells = 0;  // the interior cells within (lx, ly) of the observation, counted one by one
                for (int jj = 1; jj <= NY; ++jj)
                    for (int ii = 1; ii <= NX; ++ii)
                        cells += std::abs(ii - p.pi[q]) <= lx && std::abs(jj - p.pj[q]) <= ly;
                w = std::max(w, cells);
            }
            EXPECT(k.wcells == w);
        }
        for (int q = 0; q < n; ++q) EXPECT(in[q] == 1);
    }
    return 0;
}

int check_fault(const std::vector<int>& i, const std::vector<int>& j, const std::vector<double>& r,
                const std::vector<double>* y, const char* text) {
    AssimPlan p;
    csim::g_err.clear();
    EXPECT(csim::assim_plan_build(NX, NY, 1.0, 1.0, 1.0, false, static_cast<int>(i.size()), i.data(), j.data(), r.data(),
                                  y ? y->data() : nullptr, &p) == CSIM_ERR_ARG);
    if (csim::g_err != text) {
        std::printf("FAILED: expected \"%s\", got \"%s\"\n", text, csim::g_err.c_str());
        return 1;
    }
    return 0;
}

}  // namespace

int main() {
    using namespace csim;
    // ---- levels, plan order, batches.  loc: 0.4 -> half-widths 0, 0.6 -> 1, 1.2 -> 2, 100 -> nx - 1, ny - 1 (one bucket)
    {
        int lx = -1, ly = -1;
        EXPECT(csim_ensemble_gc_table(1.0, 1.0, 0.4, NX, NY, &lx, &ly, nullptr) == CSIM_OK && lx == 0 && ly == 0);
        EXPECT(csim_ensemble_gc_table(1.0, 1.0, 0.6, NX, NY, &lx, &ly, nullptr) == CSIM_OK && lx == 1 && ly == 1);
        EXPECT(csim_ensemble_gc_table(1.0, 1.0, 1.2, NX, NY, &lx, &ly, nullptr) == CSIM_OK && lx == 2 && ly == 2);
        EXPECT(csim_ensemble_gc_table(1.0, 1.0, 100.0, NX, NY, &lx, &ly, nullptr) == CSIM_OK && lx == NX - 1 && ly == NY - 1);
        int nl = -1;
        EXPECT(csim_ensemble_assim_plan(0, nullptr, nullptr, 1, 1, 0, nullptr, &nl) == CSIM_OK && nl == 0);
        EXPECT(csim_ensemble_assim_plan(0, nullptr, nullptr, 1, 1, 1, nullptr, &nl) == CSIM_OK && nl == 0);
    }
    const std::vector<Case> cases = {
        {{}, {}},
        {{3}, {2}},
        {{1, NX}, {1, NY}},                         // the first and the last interior cell
        {{2, 4}, {3, 3}},                           // 2 lx apart at lx = 1: they conflict
        {{2, 5}, {3, 3}},                           // 2 lx + 1 apart at lx = 1: they do not
        {{3, 7}, {2, 2}},                           // 2 lx apart at lx = 2
        {{3, 8}, {2, 2}},                           // 2 lx + 1 apart at lx = 2
        {{4, 4, 4, 4, 4, 4, 4, 4, 4}, {3, 3, 3, 3, 3, 3, 3, 3, 3}},  // one cell: nlevels == nobs
        {{1, 8, 4, 4, 2, 5, 7, 3, 1}, {1, 6, 3, 3, 5, 2, 4, 6, 6}},
        {{8, 6, 4, 2, 1, 3, 5, 7, 8}, {6, 1, 5, 2, 4, 3, 6, 1, 1}},
    };
    for (const Case& c : cases)
        for (double loc : {0.4, 0.6, 1.2, 100.0})
            for (bool ordered : {false, true})
                if (check_case(c, loc, ordered)) {
                    std::printf("  in the case of %zu observations, loc %g, ordered %d\n", c.i.size(), loc, int(ordered));
                    return 1;
                }
    {   // what the cases above are there for
        AssimPlan p;
        const std::vector<double> r(9, 1.0);
        const Case& same = cases[7];
        EXPECT(assim_plan_build(NX, NY, 1.0, 1.0, 0.4, false, 9, same.i.data(), same.j.data(), r.data(), nullptr, &p) ==
               CSIM_OK && p.nlevels == 9);
        EXPECT(assim_plan_build(NX, NY, 1.0, 1.0, 0.6, false, 2, cases[3].i.data(), cases[3].j.data(), r.data(), nullptr,
                                &p) == CSIM_OK && p.nlevels == 2);
        EXPECT(assim_plan_build(NX, NY, 1.0, 1.0, 0.6, false, 2, cases[4].i.data(), cases[4].j.data(), r.data(), nullptr,
                                &p) == CSIM_OK && p.nlevels == 1);
        EXPECT(assim_plan_build(NX, NY, 1.0, 1.0, 0.4, true, 0, nullptr, nullptr, nullptr, nullptr, &p) == CSIM_OK &&
               p.nlevels == 0 && p.off.size() == 1 && p.off[0] == 0 && p.idx.empty());
    }
    // ---- the layout of the one-shot analysis: 256-byte multiples, ascending, none overlaps
    for (size_t n : {size_t(0), size_t(1), size_t(3), size_t(257)}) {
        const size_t tcells = 63, hp = 5 * n;
        const AssimLayout l = assim_layout(n, tcells, hp);
        const size_t at[] = {l.y, l.r, l.rho, l.i, l.j, l.idx, l.scal, l.prior, l.post, l.hp, l.total};
        const size_t need[] = {8 * n, 8 * n, 8 * tcells, 4 * n, 4 * n, 4 * n, 24 * n, 16 * n, 16 * n, 8 * hp};
        for (int k = 0; k < 10; ++k) EXPECT(at[k] % 256 == 0 && at[k] + need[k] <= at[k + 1]);
        EXPECT(l.y == 0 && l.staged == l.scal && l.total % 256 == 0);
    }
    EXPECT(up(0) == 0 && up(1) == 256 && up(256) == 256 && up(257) == 512);
    // ---- every per-observation fault: its code and text; the earlier observation first; in one observation the
    // interior, then y, then r
    {
        const char* const OUTSIDE = "observation outside the interior";
        const char* const VALUE = "observation value must be finite";
        const char* const VAR = "observation error variance must be finite and > 0";
        const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
        const std::vector<int> i = {2, 5, 7}, j = {3, 1, 6};
        const std::vector<double> r = {0.5, 1.0, 2.0}, y = {0.0, -1.0, 1.0};
        for (int o = 0; o < 3; ++o) {
            for (int bad : {0, NX + 1, -3}) {
                std::vector<int> b = i;
                b[o] = bad;
                EXPECT(check_fault(b, j, r, &y, OUTSIDE) == 0 && check_fault(b, j, r, nullptr, OUTSIDE) == 0);
            }
            for (int bad : {0, NY + 1}) {
                std::vector<int> b = j;
                b[o] = bad;
                EXPECT(check_fault(i, b, r, &y, OUTSIDE) == 0);
            }
            for (double bad : {nan, inf, -inf}) {
                std::vector<double> b = y;
                b[o] = bad;
                EXPECT(check_fault(i, j, r, &b, VALUE) == 0);
            }
            for (double bad : {nan, inf, 0.0, -1.0}) {
                std::vector<double> b = r;
                b[o] = bad;
                EXPECT(check_fault(i, j, b, &y, VAR) == 0 && check_fault(i, j, b, nullptr, VAR) == 0);
            }
        }
        // two observations at fault: the earlier one's text
        const std::vector<double> y0 = {nan, -1.0, 1.0}, y2 = {0.0, -1.0, nan};
        EXPECT(check_fault(i, j, {0.5, -1.0, 2.0}, &y2, VAR) == 0);
        EXPECT(check_fault({2, 5, 0}, j, {0.5, 0.0, 2.0}, &y, VAR) == 0);
        EXPECT(check_fault({2, 5, 0}, j, r, &y0, VALUE) == 0);
        EXPECT(check_fault({2, 0, 7}, j, {0.5, 1.0, nan}, &y, OUTSIDE) == 0);
        // one observation with two or three faults
        const std::vector<double> ybad = {0.0, nan, 1.0}, rbad = {0.5, 0.0, 2.0};
        EXPECT(check_fault({2, 9, 7}, j, rbad, &ybad, OUTSIDE) == 0);
        EXPECT(check_fault({2, 9, 7}, j, r, &ybad, OUTSIDE) == 0);
        EXPECT(check_fault({2, 9, 7}, j, rbad, &y, OUTSIDE) == 0);
        EXPECT(check_fault(i, j, rbad, &ybad, VALUE) == 0);
        EXPECT(check_fault(i, j, rbad, nullptr, VAR) == 0);  // a network gives no y: nothing is read there
        // a plan that failed its half-widths says so: the table's own checks
        AssimPlan p;
        EXPECT(assim_plan_build(NX, NY, 1.0, 1.0, 0.0, false, 3, i.data(), j.data(), r.data(), nullptr, &p) == CSIM_ERR_ARG &&
               g_err == "loc must be finite and > 0");
    }
    std::printf("assim plan host ok\n");
    return 0;
}
