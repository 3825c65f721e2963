// test_spatial.cpp — neighbourhood and probability verification through climate::Ensemble
// (include/climate/ensemble.hpp) on a GPU: the displaced-hotspot case (a 67 x 48 grid, five members whose hotspot sits
// six to ten cells from the truth's).  The integer tables are compared with a plain loop over the downloaded members,
// the Fractions Skill Score must rise with the scale and cross 0.5 between half-widths 4 and 8, and the capture gives
// what the synchronous call gives.  Prints "spatial ok" and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdio>

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

typedef unsigned long long u64;

int main() {
    const int M = 5, nx = 67, ny = 48, nx2 = nx + 2, bc[4] = {0, 0, 0, 0};
    const std::size_t cells = static_cast<std::size_t>(nx2) * (ny + 2);
    const auto bump = [&](double* f, int ci, int cj) {
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                f[static_cast<std::size_t>(j + 1) * nx2 + (i + 1)] =
                    std::exp(-static_cast<double>((i - ci) * (i - ci) + (j - cj) * (j - cj)) / 18.0);
    };
    std::vector<double> truth(cells, 0.0), X(M * cells, 0.0);
    bump(truth.data(), 30, 24);
    for (int k = 0; k < M; ++k) bump(X.data() + k * cells, 36 + k, 23 + k % 3);
    const std::vector<double> thr = {0.5, 0.1};
    const std::vector<int> half = {0, 1, 2, 4, 8, 16, 32};
    const std::size_t nt = thr.size(), ns = half.size();

    climate::Ensemble e(M, nx, ny, 1.0, 1.0, bc);
    e.upload_all(X);
    const climate::SpatialVerification r = e.verify_spatial(truth, thr, half);
    EXPECT(r.thresholds == nt && r.scales == ns && r.forecast == static_cast<std::size_t>(M));
    EXPECT(r.cells == static_cast<u64>(nx) * ny && r.nan_cells == 0);

    // the definition, on the downloaded members
    const std::vector<double> D = e.download_all();
    EXPECT(D == X);
    std::vector<u64> table(nt * (M + 1) * 2, 0), nbh(nt * ns * 3, 0);
    std::vector<long> n(static_cast<std::size_t>(nx) * ny), o(n.size());
    for (std::size_t q = 0; q < nt; ++q) {
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                const std::size_t c = static_cast<std::size_t>(j + 1) * nx2 + (i + 1);
                long cnt = 0;
                for (int k = 0; k < M; ++k) cnt += D[k * cells + c] > thr[q];
                n[static_cast<std::size_t>(j) * nx + i] = cnt;
                o[static_cast<std::size_t>(j) * nx + i] = truth[c] > thr[q];
                ++table[(q * (M + 1) + cnt) * 2 + (truth[c] > thr[q])];
            }
        for (std::size_t s = 0; s < ns; ++s)
            for (int j = 0; j < ny; ++j)
                for (int i = 0; i < nx; ++i) {
                    long F = 0, O = 0;
                    for (int jj = std::max(0, j - half[s]); jj <= std::min(ny - 1, j + half[s]); ++jj)
                        for (int ii = std::max(0, i - half[s]); ii <= std::min(nx - 1, i + half[s]); ++ii) {
                            F += n[static_cast<std::size_t>(jj) * nx + ii];
                            O += o[static_cast<std::size_t>(jj) * nx + ii];
                        }
                    nbh[(q * ns + s) * 3] += static_cast<u64>(F * F);
                    nbh[(q * ns + s) * 3 + 1] += static_cast<u64>(O * O);
                    nbh[(q * ns + s) * 3 + 2] += static_cast<u64>(F * O);
                }
    }
    EXPECT(r.table == table);
    EXPECT(r.nbh == nbh);

    // skill comes with scale: nothing at the grid, useful between half-widths 4 and 8
    for (std::size_t s = 1; s < ns; ++s) EXPECT(r.scores.fss[0][s] > r.scores.fss[0][s - 1]);
    EXPECT(r.scores.fss[0][0] < 0.02 && r.scores.fss[0][3] < 0.5 && r.scores.fss[0][4] > 0.5 && r.scores.fss[0][6] > 0.9);
    for (std::size_t q = 0; q < nt; ++q) {
        const double b = r.scores.reliability[q] - r.scores.resolution[q] + r.scores.uncertainty[q];
        EXPECT(std::fabs(r.scores.brier[q] - b) <= 1e-12);
        EXPECT(r.scores.roc_area[q] >= 0.0 && r.scores.roc_area[q] <= 1.0);
        EXPECT(r.hit_rate[q * (M + 1)] == 1.0 && r.false_alarm[q * (M + 1)] == 1.0);
    }

    // the capture: the same tables, with a run and a plain verification in between
    const std::vector<double> zero(M, 0.0), dt(M, 0.1), vx(M, 0.5);
    e.set_physics(zero, dt, vx, zero);
    e.verify_spatial_begin(truth, thr, half);
    e.verify_begin(truth, {0.5});
    e.run(8);
    const climate::SpatialVerification w = e.verify_spatial_wait();
    EXPECT(w.table == table && w.nbh == nbh && w.cells == r.cells && w.nan_cells == 0);
    EXPECT(w.scores.fss[0][4] == r.scores.fss[0][4] && w.scores.brier[1] == r.scores.brier[1]);
    EXPECT(e.verify_wait().scores.cells == static_cast<long long>(r.cells));
    EXPECT(throws([&] { e.verify_spatial_wait(); }));  // nothing in flight

    // member 0 as the truth: four forecast members
    const climate::SpatialVerification m = e.verify_spatial_member(0, {0.5}, {2});
    EXPECT(m.forecast == 4 && m.table.size() == 10 && m.cells == r.cells);
    EXPECT(throws([&] { e.verify_spatial(truth, {}, half); }));       // no threshold
    EXPECT(throws([&] { e.verify_spatial(truth, thr, {33}); }));      // a half-width past 32
    EXPECT(throws([&] { e.verify_spatial_member(M, thr, half); }));   // no such member
    EXPECT(climate::verify_spatial_limit(M, nx, ny, 32) && !climate::verify_spatial_limit(4096, 125, 125, 32));

    std::printf("spatial ok\n");
    return 0;
}
