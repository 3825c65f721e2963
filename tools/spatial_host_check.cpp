// tools/spatial_host_check.cpp — the host-only code of the neighbourhood and probability verification under
// AddressSanitizer and UndefinedBehaviorSanitizer (tools/obsop_sanitize.sh): csim_verify_spatial_limit at the edge of
// its bound and csim_verify_spatial_finish on random, degenerate and largest tables (csrc/spatial_scores.cpp).  A
// stand-alone program: no device, no HIP, nothing loaded into another process.  Tables and the ROC arrays are heap
// blocks of exactly the documented size, so a read or write past them is caught.  Prints "spatial host ok" and
// returns 0, or says what failed.
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "spatial_scores.hpp"

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

typedef unsigned long long u64;

int main() {
    // ---- the bound: the largest nx ny that satisfies M^2 w^4 nx ny <= 2^62, and one more row
    for (int M : {2, 5, 63, 64, 1000, 4096})
        for (int half : {0, 1, 8, 31, 32}) {
            const u64 w = 2 * static_cast<u64>(half) + 1, per = static_cast<u64>(M) * M * w * w * w * w;
            const u64 most = (1ull << 62) / per;
            const u64 nx = most < 1000000000ull ? (most < 1000 ? most : 1000) : (1ull << 30), ny = most / nx;
            EXPECT(ny >= 1 && ny < 2147483646ull);
            EXPECT(csim_verify_spatial_limit(M, static_cast<int>(nx), static_cast<int>(ny), half) == CSIM_OK);
            EXPECT(csim_verify_spatial_limit(M, static_cast<int>(nx), static_cast<int>(ny) + 1, half) == CSIM_ERR_UNSUPPORTED);
        }
    EXPECT(csim_verify_spatial_limit(1, 2147483647, 2147483647, 0) == CSIM_OK);  // 2^62 - 2^32 + 1 cells
    EXPECT(csim_verify_spatial_limit(2, 2147483647, 2147483647, 0) == CSIM_ERR_UNSUPPORTED);
    EXPECT(csim_verify_spatial_limit(4096, 2147483647, 2147483647, 32) == CSIM_ERR_UNSUPPORTED);
    EXPECT(csim_verify_spatial_limit(4097, 1, 1, 0) == CSIM_ERR_UNSUPPORTED);
    EXPECT(csim_verify_spatial_limit(2147483647, 1, 1, 0) == CSIM_ERR_UNSUPPORTED);
    EXPECT(csim_verify_spatial_limit(0, 1, 1, 0) == CSIM_ERR_ARG && csim_verify_spatial_limit(1, 0, 1, 0) == CSIM_ERR_ARG);
    EXPECT(csim_verify_spatial_limit(1, 1, -1, 0) == CSIM_ERR_ARG && csim_verify_spatial_limit(1, 1, 1, -1) == CSIM_ERR_ARG);
    EXPECT(csim_verify_spatial_limit(1, 1, 1, 33) == CSIM_ERR_ARG);

    // ---- the finishing: random tables of every size class, the arrays exactly as large as documented
    std::mt19937_64 gen(3);
    for (int M : {1, 2, 5, 64, 4096})
        for (int nt : {1, 3, 16})
            for (int ns : {0, 1, 8}) {
                const std::size_t bins = static_cast<std::size_t>(M) + 1;
                std::vector<u64> table(nt * bins * 2), nbh(static_cast<std::size_t>(nt) * ns * 3);
                std::vector<double> hit(nt * bins), fa(nt * bins);
                u64 cells = 0;
                for (int q = 0; q < nt; ++q) {  // every threshold's table holds the same number of cells
                    u64 left = 100000;
                    for (std::size_t b = 0; b + 1 < 2 * bins; ++b) {
                        const u64 take = gen() % (left / 4 + 1);
                        table[q * 2 * bins + b] = take;
                        left -= take;
                    }
                    table[q * 2 * bins + 2 * bins - 1] = left;
                    cells = 100000;
                    for (int s = 0; s < ns; ++s) {  // half = 0: A = sum k^2 N_k, Bo = sum O_k, C = sum k O_k
                        u64 A = 0, Bo = 0, C = 0;
                        for (std::size_t k = 0; k < bins; ++k) {
                            const u64 t0 = table[(q * bins + k) * 2], t1 = table[(q * bins + k) * 2 + 1];
                            A += k * k * (t0 + t1), Bo += t1, C += k * t1;
                        }
                        nbh[(static_cast<std::size_t>(q) * ns + s) * 3] = A;
                        nbh[(static_cast<std::size_t>(q) * ns + s) * 3 + 1] = Bo;
                        nbh[(static_cast<std::size_t>(q) * ns + s) * 3 + 2] = C;
                    }
                }
                csim_spatial_scores sc;
                EXPECT(csim_verify_spatial_finish(M, nt, ns, table.data(), ns ? nbh.data() : nullptr, cells, 7, &sc,
                                                  hit.data(), fa.data()) == CSIM_OK);
                EXPECT(sc.cells == 100000 && sc.nan_cells == 7);
                for (int q = 0; q < nt; ++q) {
                    const double b = sc.reliability[q] - sc.resolution[q] + sc.uncertainty[q];
                    EXPECT(std::fabs(sc.brier[q] - b) <= 1e-12);
                    EXPECT(sc.roc_area[q] >= 0.0 && sc.roc_area[q] <= 1.0);
                    EXPECT(hit[q * bins] == 1.0 && fa[q * bins] == 1.0);
                    for (int s = 0; s < ns; ++s) EXPECT(sc.fss[q][s] >= 0.0 && sc.fss[q][s] <= 1.0);
                }
                for (int q = nt; q < CSIM_VERIFY_MAX_THRESHOLDS; ++q) EXPECT(sc.brier[q] == 0.0 && sc.fss[q][0] == 0.0);
                // without the ROC arrays, and without cells
                EXPECT(csim_verify_spatial_finish(M, nt, ns, table.data(), ns ? nbh.data() : nullptr, cells, 0, &sc,
                                                  nullptr, nullptr) == CSIM_OK);
                std::vector<u64> zt(table.size(), 0), zn(nbh.size(), 0);
                EXPECT(csim_verify_spatial_finish(M, nt, ns, zt.data(), ns ? zn.data() : nullptr, 0, 9, &sc, hit.data(),
                                                  fa.data()) == CSIM_OK);
                EXPECT(std::isnan(sc.brier[0]) && std::isnan(sc.roc_area[nt - 1]) && std::isnan(hit[nt * bins - 1]));
                if (ns) EXPECT(std::isnan(sc.fss[nt - 1][ns - 1]));
            }

    // ---- the largest sums the bound allows: S = A + M^2 Bo = 2^63 and D = S - 2 M C = 0 stay inside 64 bits
    {
        const int M = 4096;
        std::vector<u64> table(static_cast<std::size_t>(M + 1) * 2, 0), nbh(3);
        table[static_cast<std::size_t>(M) * 2 + 1] = 1ull << 38;  // every cell: all members and the truth exceed
        nbh[0] = 1ull << 62, nbh[1] = 1ull << 38, nbh[2] = 1ull << 50;
        csim_spatial_scores sc;
        EXPECT(csim_verify_spatial_finish(M, 1, 1, table.data(), nbh.data(), 1ull << 38, 0, &sc, nullptr, nullptr) == CSIM_OK);
        EXPECT(sc.fss[0][0] == 1.0 && sc.brier[0] == 0.0 && std::isnan(sc.roc_area[0]));
    }
    // ---- refusals
    {
        u64 t[4] = {1, 0, 0, 1};
        csim_spatial_scores sc;
        EXPECT(csim_verify_spatial_finish(0, 1, 0, t, nullptr, 2, 0, &sc, nullptr, nullptr) == CSIM_ERR_ARG);
        EXPECT(csim_verify_spatial_finish(1, 0, 0, t, nullptr, 2, 0, &sc, nullptr, nullptr) == CSIM_ERR_ARG);
        EXPECT(csim_verify_spatial_finish(1, 17, 0, t, nullptr, 2, 0, &sc, nullptr, nullptr) == CSIM_ERR_ARG);
        EXPECT(csim_verify_spatial_finish(1, 1, 9, t, t, 2, 0, &sc, nullptr, nullptr) == CSIM_ERR_ARG);
        EXPECT(csim_verify_spatial_finish(1, 1, 1, t, nullptr, 2, 0, &sc, nullptr, nullptr) == CSIM_ERR_ARG);
        EXPECT(csim_verify_spatial_finish(1, 1, 0, nullptr, nullptr, 2, 0, &sc, nullptr, nullptr) == CSIM_ERR_ARG);
        EXPECT(csim_verify_spatial_finish(1, 1, 0, t, nullptr, 2, 0, nullptr, nullptr, nullptr) == CSIM_ERR_ARG);
        EXPECT(csim_verify_spatial_finish(1, 1, 0, t, nullptr, 2, 0, &sc, nullptr, nullptr) == CSIM_OK);
        EXPECT(sc.brier[0] == 0.0 && sc.roc_area[0] == 1.0);  // a perfect forecast
    }
    std::printf("spatial host ok\n");
    return 0;
}
