// assim_plan.cpp — the analysis plan on the host (assim_plan.hpp): the Gaspari-Cohn table that the analysis and the
// perturbation taps share, the levels, the plan order and its batches, and the lookups of the local analysis and of the
// LETKF, one counting sort (lookup_build) behind both.  No device, no HIP headers.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <unordered_map>

#include "assim_plan.hpp"
#include "letkf_nodes.hpp"

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

// an inclusive rectangle of cells or of bins; empty where x0 > x1 or y0 > y1
struct Rect {
    int x0, x1, y0, y1;
};

// the window of the observation at plan position q, clipped to the interior
Rect window_of(int nx, int ny, const AssimPlan& p, int q) {
    const long long i = p.pi[q], j = p.pj[q];
    return {static_cast<int>(std::max(1LL, i - p.lx)), static_cast<int>(std::min<long long>(nx, i + p.lx)),
            static_cast<int>(std::max(1LL, j - p.ly)), static_cast<int>(std::min<long long>(ny, j + p.ly))};
}

// The lookup of local_tiles_build and letkf_lookup_build, a counting sort: bin y * width + x of `bins` bins lists the
// plan positions q with (x, y) in bins_of(q), sorted by input index; bin b's are pos[start[b]] .. pos[start[b + 1] - 1].
// False: more than 2^31 - 1 entries.
template <class F>
bool lookup_build(const AssimPlan& p, size_t bins, int width, std::vector<int>* start, std::vector<int>* pos, F&& bins_of) {
    std::vector<long long> cnt(bins + 1, 0);
    for (int q = 0; q < p.nobs; ++q) {
        const Rect s = bins_of(q);
        for (int y = s.y0; y <= s.y1; ++y)
            for (int x = s.x0; x <= s.x1; ++x) ++cnt[static_cast<size_t>(y) * width + x + 1];
    }
    for (size_t b = 0; b < bins; ++b) cnt[b + 1] += cnt[b];
    if (cnt[bins] > 0x7fffffffLL) return false;
    start->assign(cnt.begin(), cnt.end());
    pos->resize(static_cast<size_t>(cnt[bins]));
    // in input order, so that every bin's list comes out sorted by input index
    std::vector<int> at(p.nobs);
    for (int q = 0; q < p.nobs; ++q) at[p.idx[q]] = q;
    std::vector<int> fill(start->begin(), start->end() - 1);
    for (int o = 0; o < p.nobs; ++o) {
        const int q = at[o];
        const Rect s = bins_of(q);
        for (int y = s.y0; y <= s.y1; ++y)
            for (int x = s.x0; x <= s.x1; ++x) (*pos)[fill[static_cast<size_t>(y) * width + x]++] = q;
    }
    return true;
}

}  // namespace

namespace csim {

void gc_fill(double dx, double dy, double loc, int lx, int ly, double* table) {
    const int tw = 2 * lx + 1;
    for (int b = -ly; b <= ly; ++b)
        for (int a = -lx; a <= lx; ++a) {
            const double ax = static_cast<double>(a) * dx, by = static_cast<double>(b) * dy;
            table[static_cast<size_t>(b + ly) * tw + (a + lx)] = gc_value(std::sqrt(ax * ax + by * by) / loc);
        }
}

int assim_plan_build(int nx, int ny, double dx, double dy, double loc, bool ordered, int nobs, const int* i,
                     const int* j, const double* r, const double* y, AssimPlan* p) {
    for (int o = 0; o < nobs; ++o) {
        OBS_REQUIRE(i[o] >= 1 && i[o] <= nx && j[o] >= 1 && j[o] <= ny, "observation outside the interior");
        OBS_REQUIRE(!y || std::isfinite(y[o]), "observation value must be finite");
        OBS_REQUIRE(std::isfinite(r[o]) && r[o] > 0, "observation error variance must be finite and > 0");
    }
    if (int rc = csim_ensemble_gc_table(dx, dy, loc, nx, ny, &p->lx, &p->ly, nullptr)) return rc;
    std::vector<int> level(nobs);
    p->nobs = nobs;
    p->nlevels = nobs ? assim_levels(nobs, i, j, p->lx, p->ly, ordered, level.data()) : 0;
    // plan order: by level, then input index (a counting sort)
    p->off.assign(p->nlevels + 1, 0);
    for (int o = 0; o < nobs; ++o) ++p->off[level[o] + 1];
    for (int L = 0; L < p->nlevels; ++L) p->off[L + 1] += p->off[L];
    p->idx.resize(nobs), p->pi.resize(nobs), p->pj.resize(nobs);
    std::vector<int> fill(p->off.begin(), p->off.end() - 1);
    for (int o = 0; o < nobs; ++o) p->idx[fill[level[o]]++] = o;
    for (int q = 0; q < nobs; ++q) p->pi[q] = i[p->idx[q]], p->pj[q] = j[p->idx[q]];
    return CSIM_OK;
}

void assim_batches(int nx, int ny, const AssimPlan& p, int batch, std::vector<AssimBatch>* out) {
    out->clear();
    for (int L = 0; L < p.nlevels; ++L)
        for (int q0 = p.off[L]; q0 < p.off[L + 1]; q0 += batch) {
            const int n = std::min(batch, p.off[L + 1] - q0);
            long wcells = 0;
            for (int q = q0; q < q0 + n; ++q) {
                const long w = std::min(nx, p.pi[q] + p.lx) - std::max(1, p.pi[q] - p.lx) + 1;
                const long hgt = std::min(ny, p.pj[q] + p.ly) - std::max(1, p.pj[q] - p.ly) + 1;
                wcells = std::max(wcells, w * hgt);
            }
            out->push_back({q0, n, wcells});
        }
}

bool local_tiles_build(int nx, int ny, const AssimPlan& p, int tile, LocalTiles* out) {
    const int ntx = (nx + tile - 1) / tile, nty = (ny + tile - 1) / tile;
    // the tiles that the clipped window meets
    const bool ok = lookup_build(p, static_cast<size_t>(ntx) * nty, ntx, &out->start, &out->pos, [&](int q) {
        const Rect w = window_of(nx, ny, p, q);
        return Rect{(w.x0 - 1) / tile, (w.x1 - 1) / tile, (w.y0 - 1) / tile, (w.y1 - 1) / tile};
    });
    if (ok) out->tile = tile, out->ntx = ntx, out->nty = nty;
    return ok;
}

bool letkf_lookup_build(int nx, int ny, const AssimPlan& p, int spacing, LetkfLookup* out) {
    const int nax = letkf_axis_nodes(nx, spacing), nay = letkf_axis_nodes(ny, spacing);
    // the nodes of an axis whose cell lies in lo .. hi: their cells increase strictly with the node
    auto range = [&](int lo, int hi, int n, int na, int* first, int* last) {
        int a0 = 0, a1 = na - 1;
        while (a0 < na && letkf_node_at(a0, spacing, n) < lo) ++a0;
        while (a1 >= 0 && letkf_node_at(a1, spacing, n) > hi) --a1;
        *first = a0, *last = a1;
    };
    const bool ok = lookup_build(p, static_cast<size_t>(nax) * nay, nax, &out->start, &out->pos, [&](int q) {
        const Rect w = window_of(nx, ny, p, q);
        Rect b;
        range(w.x0, w.x1, nx, nax, &b.x0, &b.x1);
        range(w.y0, w.y1, ny, nay, &b.y0, &b.y1);
        return b;
    });
    if (ok) out->spacing = spacing, out->nax = nax, out->nay = nay;
    return ok;
}

}  // namespace csim

extern "C" {

int csim_letkf_nodes(int nx, int ny, int spacing, int* nax, int* nay, int* xi, int* yj) {
    OBS_REQUIRE(nx >= 1 && ny >= 1, "empty grid");
    OBS_REQUIRE(spacing >= 1, "spacing must be >= 1");
    const int na = letkf_axis_nodes(nx, spacing), nb = letkf_axis_nodes(ny, spacing);
    if (nax) *nax = na;
    if (nay) *nay = nb;
    for (int a = 0; xi && a < na; ++a) xi[a] = letkf_node_at(a, spacing, nx);
    for (int b = 0; yj && b < nb; ++b) yj[b] = letkf_node_at(b, spacing, ny);
    return CSIM_OK;
}

int csim_letkf_blend(int nx, int ny, int spacing, int i, int j, int node[4], double beta[4]) {
    OBS_REQUIRE(nx >= 1 && ny >= 1, "empty grid");
    OBS_REQUIRE(spacing >= 1, "spacing must be >= 1");
    OBS_REQUIRE(i >= 1 && i <= nx && j >= 1 && j <= ny, "cell outside the interior");
    OBS_REQUIRE(node && beta, "null argument");
    const int na = letkf_axis_nodes(nx, spacing), nb = letkf_axis_nodes(ny, spacing);
    const LetkfAxis x = letkf_axis_blend(i, spacing, nx, na), y = letkf_axis_blend(j, spacing, ny, nb);
    const int a1 = std::min(x.a + 1, na - 1), b1 = std::min(y.a + 1, nb - 1);
    node[0] = y.a * na + x.a, node[1] = y.a * na + a1, node[2] = b1 * na + x.a, node[3] = b1 * na + a1;
    letkf_weights4(x.t, y.t, beta);
    return CSIM_OK;
}

int csim_letkf_plan(int M, int nx, int ny, int spacing, long* nodes, long long* bytes) {
    OBS_REQUIRE(M >= 2, "M must be >= 2");
    OBS_REQUIRE(nx >= 1 && ny >= 1, "empty grid");
    OBS_REQUIRE(spacing >= 1, "spacing must be >= 1");
    if (M > CSIM_ESPACE_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_letkf_plan: at most CSIM_ESPACE_MAX_MEMBERS forecast members");
    const long nn = static_cast<long>(letkf_axis_nodes(nx, spacing)) * letkf_axis_nodes(ny, spacing);
    if (nodes) *nodes = nn;
    if (bytes) *bytes = static_cast<long long>(letkf_layout(M, nn, eigen_device_form(M, 0)).bytes);
    return CSIM_OK;
}

int csim_ensemble_gc_table(double dx, double dy, double loc, int nx, int ny, int* lx, int* ly, double* table) {
    OBS_REQUIRE(lx && ly, "null argument");
    OBS_REQUIRE(std::isfinite(dx) && dx > 0 && std::isfinite(dy) && dy > 0, "dx/dy must be finite and > 0");
    OBS_REQUIRE(std::isfinite(loc) && loc > 0, "loc must be finite and > 0");
    OBS_REQUIRE(nx >= 1 && ny >= 1, "empty grid");
    *lx = gc_half(dx, loc, nx);
    *ly = gc_half(dy, loc, ny);
    if (table) gc_fill(dx, dy, loc, *lx, *ly, table);
    return CSIM_OK;
}

int csim_ensemble_assim_plan(int nobs, const int* i, const int* j, int lx, int ly, int ordered, int* level,
                             int* nlevels) {
    OBS_REQUIRE(nlevels, "null nlevels");
    OBS_REQUIRE(nobs >= 0, "nobs must be >= 0");
    OBS_REQUIRE(nobs == 0 || (i && j && level), "null array");
    OBS_REQUIRE(lx >= 0 && ly >= 0, "lx and ly must be >= 0");
    OBS_REQUIRE(ordered == 0 || ordered == 1, "ordered must be 0 or 1");
    if (nobs > CSIM_ASSIM_MAX_OBS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assim_plan: at most 2^20 observations");
    *nlevels = assim_levels(nobs, i, j, lx, ly, ordered == 1, level);
    return CSIM_OK;
}

int csim_obs_local_count(int nx, int ny, int nobs, const int* i, const int* j, int lx, int ly, int* count,
                         int* max_local) {
    OBS_REQUIRE(nx >= 1 && ny >= 1, "empty grid");
    OBS_REQUIRE(nobs >= 0, "nobs must be >= 0");
    OBS_REQUIRE(nobs == 0 || (i && j), "null array");
    OBS_REQUIRE(lx >= 0 && ly >= 0, "lx and ly must be >= 0");
    for (int o = 0; o < nobs; ++o)
        OBS_REQUIRE(i[o] >= 1 && i[o] <= nx && j[o] >= 1 && j[o] <= ny, "observation outside the interior");
    // a 2-D difference array with one spare row and column: +1 at the rectangle's first corner, -1 past its ends
    const size_t w = static_cast<size_t>(nx) + 1;
    std::vector<int> d(w * (static_cast<size_t>(ny) + 1), 0);
    for (int o = 0; o < nobs; ++o) {
        const size_t i0 = static_cast<size_t>(std::max(1LL, static_cast<long long>(i[o]) - lx)) - 1;
        const size_t i1 = static_cast<size_t>(std::min<long long>(nx, static_cast<long long>(i[o]) + lx));
        const size_t j0 = static_cast<size_t>(std::max(1LL, static_cast<long long>(j[o]) - ly)) - 1;
        const size_t j1 = static_cast<size_t>(std::min<long long>(ny, static_cast<long long>(j[o]) + ly));
        ++d[j0 * w + i0], --d[j0 * w + i1], --d[j1 * w + i0], ++d[j1 * w + i1];
    }
    int most = 0;
    for (size_t b = 0; b < static_cast<size_t>(ny); ++b)
        for (size_t a = 0; a < static_cast<size_t>(nx); ++a) {
            long long v = d[b * w + a];  // at most nobs, its parts up to twice that
            if (a) v += d[b * w + a - 1];
            if (b) v += d[(b - 1) * w + a];
            if (a && b) v -= d[(b - 1) * w + a - 1];
            d[b * w + a] = static_cast<int>(v);
            most = std::max(most, static_cast<int>(v));
            if (count) count[b * static_cast<size_t>(nx) + a] = static_cast<int>(v);
        }
    if (max_local) *max_local = most;
    return CSIM_OK;
}

int csim_ensemble_perturb_taps(double d, double corr_len, int n, int periodic, int* R, double* taps) {
    OBS_REQUIRE(R, "null argument");
    OBS_REQUIRE(std::isfinite(d) && d > 0, "the spacing must be finite and > 0");
    OBS_REQUIRE(std::isfinite(corr_len) && corr_len >= 0, "corr_len must be finite and >= 0");
    OBS_REQUIRE(n >= 1, "empty axis");
    OBS_REQUIRE(periodic == 0 || periodic == 1, "periodic must be 0 or 1");
    *R = perturb_radius(d, corr_len, n, periodic == 1);
    if (*R > CSIM_PERTURB_MAX_RADIUS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_perturb_taps: the radius exceeds CSIM_PERTURB_MAX_RADIUS");
    if (taps) perturb_fill(d, corr_len, *R, taps);
    return CSIM_OK;
}

}  // extern "C"
