// ensemble_da.cpp — the ensemble's data assimilation: the EnSRF analysis and its plan, the seeded perturbations and the
// RTPS / RTPP relaxation (kernels in ensemble_assim.hip, ensemble_perturb.hip, ensemble_relax.hip; random numbers in
// ensemble_noise.hpp), with the Gaspari-Cohn table that the analysis and the perturbation taps share.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <unordered_map>
#include <vector>

#include "ensemble_host.hpp"
#include "ensemble_noise.hpp"

using namespace csim;

namespace {

// the localisation half-width along one axis: the largest a >= 0 with a * h < 2 loc, at most n - 1
int gc_half(double h, double loc, int n) {
    const double s = 2.0 * loc;
    if (static_cast<double>(n - 1) * h < s) return n - 1;
    int a = static_cast<int>(std::min(std::floor(s / h), static_cast<double>(n - 1)));
    while (a > 0 && static_cast<double>(a) * h >= s) --a;
    while (a + 1 < n && static_cast<double>(a + 1) * h < s) ++a;
    return a;
}

// Gaspari-Cohn in the Horner forms of csim.h, clamped at +0
double gc_value(double z) {
    double v = 0.0;
    if (z <= 1.0)
        v = ((((-0.25 * z + 0.5) * z + 0.625) * z - 5.0 / 3.0) * z) * z + 1.0;
    else if (z < 2.0)
        v = ((((z / 12.0 - 0.5) * z + 0.625) * z + 5.0 / 3.0) * z - 5.0) * z + 4.0 - 2.0 / (3.0 * z);
    return v > 0.0 ? v : 0.0;
}

void gc_fill(double dx, double dy, double loc, int lx, int ly, double* table) {
    const int tw = 2 * lx + 1;
    for (int b = -ly; b <= ly; ++b)
        for (int a = -lx; a <= lx; ++a) {
            const double ax = static_cast<double>(a) * dx, by = static_cast<double>(b) * dy;
            table[static_cast<size_t>(b + ly) * tw + (a + lx)] = gc_value(std::sqrt(ax * ax + by * by) / loc);
        }
}

// the smoothing taps of csim_ensemble_perturb along one axis (csim_ensemble_perturb_taps): the radius, and with `taps`
// the 2 R + 1 Gaspari-Cohn weights scaled to unit sum of squares
int perturb_radius(double d, double c, int n, bool periodic) {
    return c == 0.0 ? 0 : gc_half(d, c, periodic ? (n - 1) / 2 + 1 : n);
}

void perturb_fill(double d, double c, int R, double* taps) {
    if (c == 0.0) {
        taps[0] = 1.0;
        return;
    }
    for (int o = -R; o <= R; ++o) taps[o + R] = gc_value(static_cast<double>(std::abs(o)) * d / c);
    double S = 0.0;
    for (int o = 0; o <= 2 * R; ++o) S = S + taps[o] * taps[o];
    const double norm = std::sqrt(S);
    for (int o = 0; o <= 2 * R; ++o) taps[o] = taps[o] / norm;
}

// the levels of csim_ensemble_assim_plan.  Spatial buckets of (2 lx + 1) x (2 ly + 1) cells: observations that
// conflict lie in the same bucket or in one of its eight neighbours.  First fit keeps one bucket map per level,
// ordered mode one for all earlier observations.
int assim_levels(int n, const int* oi, const int* oj, int lx, int ly, bool ordered, int* level) {
    const long long wx = 2LL * lx, wy = 2LL * ly;
    auto bucket = [&](long long v, long long w) { return v >= 0 ? v / (w + 1) : -((-v + w) / (w + 1)); };
    auto key = [](long long bi, long long bj) { return static_cast<unsigned long long>(bi) * 0x9E3779B97F4A7C15ull ^
                                                       static_cast<unsigned long long>(bj); };
    using Map = std::unordered_map<unsigned long long, std::vector<int>>;
    // calls f(p) for every observation p of map m in the 3 x 3 buckets around o that conflicts with o; stops when f
    // returns true
    auto scan = [&](const Map& m, int o, auto&& f) {
        const long long bi = bucket(oi[o], wx), bj = bucket(oj[o], wy);
        for (long long u = bi - 1; u <= bi + 1; ++u)
            for (long long v = bj - 1; v <= bj + 1; ++v) {
                auto it = m.find(key(u, v));
                if (it == m.end()) continue;
                for (int p : it->second)
                    if (std::llabs(static_cast<long long>(oi[p]) - oi[o]) <= wx &&
                        std::llabs(static_cast<long long>(oj[p]) - oj[o]) <= wy && f(p))
                        return;
            }
    };
    int nl = 0;
    if (ordered) {
        Map all;
        for (int o = 0; o < n; ++o) {
            int lv = 0;
            scan(all, o, [&](int p) {
                lv = std::max(lv, level[p] + 1);
                return false;
            });
            level[o] = lv;
            nl = std::max(nl, lv + 1);
            all[key(bucket(oi[o], wx), bucket(oj[o], wy))].push_back(o);
        }
        return nl;
    }
    std::vector<Map> per;
    for (int o = 0; o < n; ++o) {
        int lv = 0;
        for (;; ++lv) {
            if (lv == static_cast<int>(per.size())) break;
            bool hit = false;
            scan(per[lv], o, [&](int) { return hit = true; });
            if (!hit) break;
        }
        if (lv == static_cast<int>(per.size())) per.emplace_back();
        per[lv][key(bucket(oi[o], wx), bucket(oj[o], wy))].push_back(o);
        level[o] = lv;
    }
    return static_cast<int>(per.size());
}

// byte layout of the analysis buffer: the staged inputs (y, r, table, i, j, input index), then the device-only
// scalars (3 per observation), prior and posterior diagnostics (2 each per observation) and one batch's h'_k
struct AssimLayout {
    size_t y, r, rho, i, j, idx, staged, scal, prior, post, hp, total;
};
AssimLayout assim_layout(size_t n, size_t tcells, size_t hp) {
    auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
    AssimLayout l{};
    l.y = 0;
    l.r = up(l.y + 8 * n);
    l.rho = up(l.r + 8 * n);
    l.i = up(l.rho + 8 * tcells);
    l.j = up(l.i + 4 * n);
    l.idx = up(l.j + 4 * n);
    l.staged = up(l.idx + 4 * n);
    l.scal = l.staged;
    l.prior = up(l.scal + 24 * n);
    l.post = up(l.prior + 16 * n);
    l.hp = up(l.post + 16 * n);
    l.total = up(l.hp + 8 * hp);
    return l;
}

// the checks csim_ensemble_prior_capture and csim_ensemble_relax share
int relax_check(const csim_ensemble* e, int mode, int truth_member, int* M, int* t) {
    CSIM_REQUIRE(mode == CSIM_RELAX_SPREAD || mode == CSIM_RELAX_PERT, "mode must be CSIM_RELAX_SPREAD or CSIM_RELAX_PERT");
    CSIM_TRY(forecast_split(e->g.members, truth_member, M, t, 2, "the relaxation needs at least two forecast members",
                            ASSIM_MAX_MEMBERS, "csim_ensemble_relax: at most 1024 forecast members"));
    CSIM_REQUIRE(e->g.slab <= 0x7fffffffL, "grid too large for the relaxation");
    return CSIM_OK;
}

}  // namespace

namespace csim {

void assim_batches(const EnsGeom& g, int nlevels, const int* off, const int* pi, const int* pj, int lx, int ly,
                   int batch, std::vector<AssimBatch>* out) {
    out->clear();
    for (int L = 0; L < nlevels; ++L)
        for (int q0 = off[L]; q0 < off[L + 1]; q0 += batch) {
            const int n = std::min(batch, off[L + 1] - q0);
            long wcells = 0;
            for (int q = q0; q < q0 + n; ++q) {
                const long w = std::min(g.nx, pi[q] + lx) - std::max(1, pi[q] - lx) + 1;
                const long hgt = std::min(g.ny, pj[q] + ly) - std::max(1, pj[q] - ly) + 1;
                wcells = std::max(wcells, w * hgt);
            }
            out->push_back({q0, n, wcells});
        }
}

int assim_enqueue(csim_ensemble* e, const AssimArgs& a, double inflation, const std::vector<AssimBatch>& batches) {
    const EnsGeom& g = e->g;
    double* f = e->base(e->cur);
    if (inflation != 1.0)
        CSIM_HIP(ens_launch_assim_inflate(g, f, a.forecast, a.truth_member, inflation - 1.0, e->st));
    for (const AssimBatch& b : batches) {
        CSIM_HIP(ens_launch_assim_prior(g, f, a, b.first, b.count, e->st));
        CSIM_HIP(ens_launch_assim_update(g, f, a, b.first, b.count, b.wcells, e->st));
    }
    return CSIM_OK;
}

}  // namespace csim

extern "C" {

int csim_ensemble_gc_table(double dx, double dy, double loc, int nx, int ny, int* lx, int* ly, double* table) {
    CSIM_REQUIRE(lx && ly, "null argument");
    CSIM_REQUIRE(std::isfinite(dx) && dx > 0 && std::isfinite(dy) && dy > 0, "dx/dy must be finite and > 0");
    CSIM_REQUIRE(std::isfinite(loc) && loc > 0, "loc must be finite and > 0");
    CSIM_REQUIRE(nx >= 1 && ny >= 1, "empty grid");
    *lx = gc_half(dx, loc, nx);
    *ly = gc_half(dy, loc, ny);
    if (table) gc_fill(dx, dy, loc, *lx, *ly, table);
    return CSIM_OK;
}

int csim_ensemble_assim_plan(int nobs, const int* i, const int* j, int lx, int ly, int ordered, int* level,
                             int* nlevels) {
    CSIM_REQUIRE(nlevels, "null nlevels");
    CSIM_REQUIRE(nobs >= 0, "nobs must be >= 0");
    CSIM_REQUIRE(nobs == 0 || (i && j && level), "null array");
    CSIM_REQUIRE(lx >= 0 && ly >= 0, "lx and ly must be >= 0");
    CSIM_REQUIRE(ordered == 0 || ordered == 1, "ordered must be 0 or 1");
    if (nobs > ASSIM_MAX_OBS) return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assim_plan: at most 2^20 observations");
    *nlevels = assim_levels(nobs, i, j, lx, ly, ordered == 1, level);
    return CSIM_OK;
}

int csim_ensemble_assimilate(csim_ensemble* e, int nobs, const int* i, const int* j, const double* y, const double* r,
                             double loc, double inflation, int truth_member, int ordered, double* prior_mean,
                             double* prior_var, double* post_mean, double* post_var, int* nlevels) {
    CSIM_REQUIRE(e, "null ensemble");
    const EnsGeom& g = e->g;
    const int B = g.members;
    CSIM_REQUIRE(nobs >= 0, "nobs must be >= 0");
    CSIM_REQUIRE(nobs == 0 || (i && j && y && r), "null observation array");
    CSIM_REQUIRE(std::isfinite(loc) && loc > 0, "loc must be finite and > 0");
    CSIM_REQUIRE(std::isfinite(inflation) && inflation >= 1.0, "inflation must be finite and >= 1");
    int M = 0, t = 0;
    CSIM_TRY(forecast_split(B, truth_member, &M, &t));
    CSIM_REQUIRE(ordered == 0 || ordered == 1, "ordered must be 0 or 1");
    CSIM_REQUIRE(M >= 2, "the analysis needs at least two forecast members");
    if (M > ASSIM_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate: at most 1024 forecast members");
    if (nobs > ASSIM_MAX_OBS) return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate: at most 2^20 observations");
    for (int o = 0; o < nobs; ++o) {
        CSIM_REQUIRE(i[o] >= 1 && i[o] <= g.nx && j[o] >= 1 && j[o] <= g.ny, "observation outside the interior");
        CSIM_REQUIRE(std::isfinite(y[o]), "observation value must be finite");
        CSIM_REQUIRE(std::isfinite(r[o]) && r[o] > 0, "observation error variance must be finite and > 0");
    }
    int lx = 0, ly = 0;
    CSIM_TRY(csim_ensemble_gc_table(e->dx, e->dy, loc, g.nx, g.ny, &lx, &ly, nullptr));
    std::vector<int> level(nobs);
    int nl = nobs ? assim_levels(nobs, i, j, lx, ly, ordered == 1, level.data()) : 0;
    if (nlevels) *nlevels = nl;
    const bool diag = prior_mean || prior_var || post_mean || post_var;
    if (nobs == 0 && inflation == 1.0) return diag ? csim_ensemble_sync(e) : CSIM_OK;

    // plan order: by level, then input index (a counting sort)
    std::vector<int> off(nl + 1, 0), ord(nobs);
    for (int o = 0; o < nobs; ++o) ++off[level[o] + 1];
    for (int L = 0; L < nl; ++L) off[L + 1] += off[L];
    {
        std::vector<int> fill(off.begin(), off.end() - 1);
        for (int o = 0; o < nobs; ++o) ord[fill[level[o]]++] = o;
    }
    const size_t tcells = static_cast<size_t>(2 * lx + 1) * (2 * ly + 1);
    const int batch = assim_batch_size(M);
    const size_t hp = static_cast<size_t>(std::min(nobs, batch)) * M;
    const AssimLayout l = assim_layout(nobs, tcells, hp);

    // resources: the device buffer grows after the work already enqueued is done with it, the staging buffer after
    // its last copy has run
    void* staged = nullptr;
    CSIM_TRY(e->assim.dev.reserve(l.total, e->st));
    CSIM_TRY(e->assim.stage.acquire(l.staged, &staged));
    char* const h = static_cast<char*>(staged);
    char* const d = e->assim.dev.as<char>();
    auto* hy = reinterpret_cast<double*>(h + l.y);
    auto* hr = reinterpret_cast<double*>(h + l.r);
    auto* hi = reinterpret_cast<int*>(h + l.i);
    auto* hj = reinterpret_cast<int*>(h + l.j);
    auto* hx = reinterpret_cast<int*>(h + l.idx);
    for (int q = 0; q < nobs; ++q) {
        const int o = ord[q];
        hy[q] = y[o], hr[q] = r[o], hi[q] = i[o], hj[q] = j[o], hx[q] = o;
    }
    gc_fill(e->dx, e->dy, loc, lx, ly, reinterpret_cast<double*>(h + l.rho));
    CSIM_TRY(e->assim.stage.send(d, l.staged, e->st));

    AssimArgs a{};
    a.forecast = M;
    a.truth_member = t;
    a.lx = lx, a.ly = ly;
    a.rho = reinterpret_cast<const double*>(d + l.rho);
    a.obs.i = reinterpret_cast<const int*>(d + l.i);
    a.obs.j = reinterpret_cast<const int*>(d + l.j);
    a.obs.idx = reinterpret_cast<const int*>(d + l.idx);
    a.obs.y = reinterpret_cast<const double*>(d + l.y);
    a.obs.r = reinterpret_cast<const double*>(d + l.r);
    a.scal = reinterpret_cast<double*>(d + l.scal);
    a.hp = reinterpret_cast<double*>(d + l.hp);
    a.prior = prior_mean || prior_var ? reinterpret_cast<double*>(d + l.prior) : nullptr;
    // a.tstart stays null: point observations
    std::vector<AssimBatch> batches;
    assim_batches(g, nl, off.data(), hi, hj, lx, ly, batch, &batches);
    CSIM_TRY(assim_enqueue(e, a, inflation, batches));
    double* f = e->base(e->cur);
    if (!diag) return CSIM_OK;
    auto* post = reinterpret_cast<double*>(d + l.post);
    if (post_mean || post_var) CSIM_HIP(ens_launch_assim_post(g, f, a, nobs, post, e->st));
    std::vector<double> pr(2 * static_cast<size_t>(nobs)), po(2 * static_cast<size_t>(nobs));
    if (a.prior && nobs)
        CSIM_HIP(hipMemcpyAsync(pr.data(), a.prior, sizeof(double) * pr.size(), hipMemcpyDeviceToHost, e->st));
    if ((post_mean || post_var) && nobs)
        CSIM_HIP(hipMemcpyAsync(po.data(), post, sizeof(double) * po.size(), hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    for (int o = 0; o < nobs; ++o) {
        if (prior_mean) prior_mean[o] = pr[2 * static_cast<size_t>(o)];
        if (prior_var) prior_var[o] = pr[2 * static_cast<size_t>(o) + 1];
        if (post_mean) post_mean[o] = po[2 * static_cast<size_t>(o)];
        if (post_var) post_var[o] = po[2 * static_cast<size_t>(o) + 1];
    }
    return CSIM_OK;
}

int csim_philox4x32(const unsigned ctr[4], const unsigned key[2], unsigned out[4]) {
    CSIM_REQUIRE(ctr && key && out, "null argument");
    unsigned c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]};
    philox4x32(c, key[0], key[1]);
    for (int k = 0; k < 4; ++k) out[k] = c[k];
    return CSIM_OK;
}

int csim_normal_from_bits(unsigned long long bits, double* z) {
    CSIM_REQUIRE(z, "null argument");
    *z = normal_from_bits(bits);
    return CSIM_OK;
}

int csim_ensemble_perturb_taps(double d, double corr_len, int n, int periodic, int* R, double* taps) {
    CSIM_REQUIRE(R, "null argument");
    CSIM_REQUIRE(std::isfinite(d) && d > 0, "the spacing must be finite and > 0");
    CSIM_REQUIRE(std::isfinite(corr_len) && corr_len >= 0, "corr_len must be finite and >= 0");
    CSIM_REQUIRE(n >= 1, "empty axis");
    CSIM_REQUIRE(periodic == 0 || periodic == 1, "periodic must be 0 or 1");
    *R = perturb_radius(d, corr_len, n, periodic == 1);
    if (*R > PERTURB_MAX_RADIUS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_perturb_taps: the radius exceeds CSIM_PERTURB_MAX_RADIUS");
    if (taps) perturb_fill(d, corr_len, *R, taps);
    return CSIM_OK;
}

int csim_ensemble_perturb(csim_ensemble* e, unsigned long long seed, unsigned draw, double sigma, double corr_len,
                          int centered, int truth_member) {
    CSIM_REQUIRE(e, "null ensemble");
    const EnsGeom& g = e->g;
    const int B = g.members;
    CSIM_REQUIRE(std::isfinite(sigma), "sigma must be finite");
    CSIM_REQUIRE(std::isfinite(corr_len) && corr_len >= 0, "corr_len must be finite and >= 0");
    CSIM_REQUIRE(centered == 0 || centered == 1, "centered must be 0 or 1");
    int M = 0, t = 0;
    CSIM_TRY(forecast_split(B, truth_member, &M, &t, 1, "no forecast member"));
    CSIM_REQUIRE(!centered || M >= 2, "centering needs at least two forecast members");
    PerturbArgs a{};
    a.perx = g.bc[CSIM_LEFT] == CSIM_BC_PERIODIC && g.bc[CSIM_RIGHT] == CSIM_BC_PERIODIC;
    a.pery = g.bc[CSIM_BOTTOM] == CSIM_BC_PERIODIC && g.bc[CSIM_TOP] == CSIM_BC_PERIODIC;
    CSIM_TRY(csim_ensemble_perturb_taps(e->dx, corr_len, g.nx, a.perx, &a.rx, a.tx));
    CSIM_TRY(csim_ensemble_perturb_taps(e->dy, corr_len, g.ny, a.pery, &a.ry, a.ty));
    if (sigma == 0.0) return CSIM_OK;
    a.seed_lo = static_cast<unsigned>(seed), a.seed_hi = static_cast<unsigned>(seed >> 32), a.draw = draw;
    a.forecast = M;
    a.truth_member = t;
    a.sigma = sigma;
    CSIM_HIP(ens_launch_perturb(g, e->base(e->cur), a, centered == 1, e->st));
    return CSIM_OK;
}

int csim_ensemble_prior_capture(csim_ensemble* e, int mode, int truth_member) {
    CSIM_REQUIRE(e, "null ensemble");
    const EnsGeom& g = e->g;
    csim_ensemble::Relax& x = e->relax;
    int M = 0, t = 0;
    CSIM_TRY(relax_check(e, mode, truth_member, &M, &t));
    // each buffer is made at the first capture that needs it
    const size_t bytes = sizeof(double) * static_cast<size_t>(g.slab) * g.members;
    CSIM_TRY(mode == CSIM_RELAX_SPREAD ? x.sb.reserve(sizeof(double) * static_cast<size_t>(g.nx) * g.ny)
                                       : x.prior.reserve(bytes));
    x.mode = 0;  // from here on the last capture is being overwritten (in stream order, after its readers)
    if (mode == CSIM_RELAX_SPREAD)
        CSIM_HIP(ens_launch_relax_capture(g, e->base(e->cur), M, t, x.sb.as(), e->st));
    else
        CSIM_HIP(hipMemcpyAsync(x.prior.p, e->alloc[e->cur], bytes, hipMemcpyDeviceToDevice, e->st));
    x.mode = mode;
    x.truth = truth_member;
    return CSIM_OK;
}

int csim_ensemble_relax(csim_ensemble* e, int mode, double alpha, int truth_member, double* out_factor) {
    CSIM_REQUIRE(e, "null ensemble");
    const EnsGeom& g = e->g;
    csim_ensemble::Relax& x = e->relax;
    int M = 0, t = 0;
    CSIM_TRY(relax_check(e, mode, truth_member, &M, &t));
    CSIM_REQUIRE(std::isfinite(alpha) && alpha >= 0.0 && alpha <= 1.0, "alpha must be in [0, 1]");
    CSIM_REQUIRE(!(out_factor && mode == CSIM_RELAX_PERT), "out_factor is for CSIM_RELAX_SPREAD only");
    if (x.mode != mode || x.truth != truth_member)
        return fail(CSIM_ERR_STATE, "csim_ensemble_relax: no valid capture of this mode and truth member "
                                    "(csim_ensemble_prior_capture after the last run)");
    const size_t cells = stats_cells(e);
    if (alpha == 0.0) {
        if (!out_factor) return CSIM_OK;
        std::fill(out_factor, out_factor + cells, 0.0);
        return csim_ensemble_sync(e);
    }
    if (out_factor) CSIM_TRY(x.factor.reserve(sizeof(double) * cells));
    // Only interior cells of the forecast members in the current buffer are written, as in csim_ensemble_assimilate:
    // ring_ok is only ever true for rings without a Neumann side, whose ghosts do not depend on the interior, Neumann
    // rings are rebuilt from the interior before every pass, and the FinLines were consumed by the ghost fill that ended
    // the run that wrote them, so nothing cached goes stale.
    if (mode == CSIM_RELAX_PERT) {
        CSIM_HIP(ens_launch_relax_pert(g, e->base(e->cur), x.prior.as() + static_cast<size_t>(GHOST_EXTRA) * g.pitch, M, t,
                                       alpha, e->st));
        return CSIM_OK;
    }
    if (out_factor) CSIM_HIP(hipMemsetAsync(x.factor.p, 0, sizeof(double) * cells, e->st));  // the ghost ring: +0
    CSIM_HIP(ens_launch_relax_spread(g, e->base(e->cur), M, t, alpha, x.sb.as(), out_factor ? x.factor.as() : nullptr,
                                     e->st));
    if (!out_factor) return CSIM_OK;
    // as csim_ensemble_stats: copied in stream order, and the call waits for it
    CSIM_HIP(hipMemcpyAsync(out_factor, x.factor.p, sizeof(double) * cells, hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    return CSIM_OK;
}

}  // extern "C"
