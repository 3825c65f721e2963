// spatial_scores.cpp — the host mathematics of the neighbourhood and probability verification (spatial_scores.hpp):
// the overflow bound of the integer sums, and the scores of the integer tables in the order csim.h fixes, so that C,
// C++ and Python derive the same bits.  No device, no HIP headers.
#include <cmath>
#include <cstring>

#include "spatial_scores.hpp"

using namespace csim;

typedef unsigned long long u64;

namespace csim {

int spatial_limit(int M, long nx, long ny, int half_max) {
    if (M > CSIM_SPATIAL_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_verify_spatial: at most 4096 forecast members");
    const u64 w = 2 * static_cast<u64>(half_max) + 1;
    const unsigned __int128 v = static_cast<unsigned __int128>(static_cast<u64>(M) * M * w * w * w * w) *
                                (static_cast<u64>(nx) * static_cast<u64>(ny));
    if (v > (static_cast<unsigned __int128>(1) << 62))
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_verify_spatial: M^2 w^4 nx ny exceeds 2^62, the sums could overflow");
    return CSIM_OK;
}

}  // namespace csim

namespace {

const double NANV = std::nan("");

// the scores of one threshold (csim.h has the formulas and their order)
void finish_threshold(int M, int ns, const u64* T, const u64* nbh, u64 n, int q, csim_spatial_scores* out, double* hit,
                      double* fa) {
    u64 SO = 0;
    for (int k = 0; k <= M; ++k) SO += T[2 * k + 1];
    const double dn = static_cast<double>(n), dM = static_cast<double>(M);
    if (n == 0) {
        out->brier[q] = out->reliability[q] = out->resolution[q] = out->uncertainty[q] = out->roc_area[q] = NANV;
        for (int k = 0; k <= M; ++k) {
            if (hit) hit[k] = NANV;
            if (fa) fa[k] = NANV;
        }
    } else {
        const double obar = static_cast<double>(SO) / dn;
        double b = 0.0, rel = 0.0, res = 0.0;
        for (int k = 0; k <= M; ++k) {
            const double p = static_cast<double>(k) / dM, pm = p - 1.0;
            const double t0 = (p * p) * static_cast<double>(T[2 * k]);
            const double t1 = (pm * pm) * static_cast<double>(T[2 * k + 1]);
            b = b + (t0 + t1);
            const u64 N = T[2 * k] + T[2 * k + 1];
            if (N > 0) {
                const double dN = static_cast<double>(N), f = static_cast<double>(T[2 * k + 1]) / dN;
                const double d1 = p - f, d2 = f - obar;
                rel = rel + dN * (d1 * d1);
                res = res + dN * (d2 * d2);
            }
        }
        out->brier[q] = b / dn;
        out->reliability[q] = rel / dn;
        out->resolution[q] = res / dn;
        out->uncertainty[q] = obar * (1.0 - obar);
        // ROC, from "at least M + 1 members" (0, 0) down to "at least 0" (1, 1)
        const bool no_event = SO == 0, no_miss = SO == n;
        const double dSO = static_cast<double>(SO), dNO = static_cast<double>(n - SO);
        u64 ch = 0, cf = 0;
        double area = 0.0, hp = 0.0, fp = 0.0;
        for (int k = M; k >= 0; --k) {
            ch += T[2 * k + 1];
            cf += T[2 * k];
            const double hk = no_event ? NANV : static_cast<double>(ch) / dSO;
            const double fk = no_miss ? NANV : static_cast<double>(cf) / dNO;
            if (hit) hit[k] = hk;
            if (fa) fa[k] = fk;
            if (!no_event && !no_miss) area = area + ((fk - fp) * (hk + hp)) * 0.5;
            hp = hk, fp = fk;
        }
        out->roc_area[q] = (no_event || no_miss) ? NANV : area;
    }
    const u64 m = static_cast<u64>(M);
    for (int s = 0; s < ns; ++s) {
        const u64 A = nbh[3 * s], Bo = nbh[3 * s + 1], C = nbh[3 * s + 2];
        const u64 S = A + m * m * Bo, D = S - 2 * m * C;
        out->fss[q][s] = S == 0 ? NANV : 1.0 - static_cast<double>(D) / static_cast<double>(S);
    }
}

}  // namespace

extern "C" {

int csim_verify_spatial_limit(int M, int nx, int ny, int half_max) {
    OBS_REQUIRE(M >= 1 && nx >= 1 && ny >= 1, "M, nx and ny must be >= 1");
    OBS_REQUIRE(half_max >= 0 && half_max <= CSIM_SPATIAL_MAX_HALF, "half_max must be 0 .. 32");
    return spatial_limit(M, nx, ny, half_max);
}

int csim_verify_spatial_finish(int M, int nt, int ns, const unsigned long long* table, const unsigned long long* nbh,
                               unsigned long long cells, unsigned long long nan_cells, csim_spatial_scores* out,
                               double* hit_rate, double* false_alarm) {
    OBS_REQUIRE(M >= 1, "M must be >= 1");
    OBS_REQUIRE(nt >= 1 && nt <= CSIM_VERIFY_MAX_THRESHOLDS, "nt must be 1 .. 16");
    OBS_REQUIRE(ns >= 0 && ns <= CSIM_SPATIAL_MAX_SCALES, "ns must be 0 .. 8");
    OBS_REQUIRE(table && out && (ns == 0 || nbh), "null argument");
    std::memset(out, 0, sizeof(*out));
    out->cells = static_cast<long long>(cells);
    out->nan_cells = static_cast<long long>(nan_cells);
    const size_t bins = static_cast<size_t>(M) + 1;
    for (int q = 0; q < nt; ++q)
        finish_threshold(M, ns, table + q * 2 * bins, ns ? nbh + static_cast<size_t>(q) * 3 * ns : nullptr, cells, q, out,
                         hit_rate ? hit_rate + q * bins : nullptr, false_alarm ? false_alarm + q * bins : nullptr);
    return CSIM_OK;
}

}  // extern "C"
