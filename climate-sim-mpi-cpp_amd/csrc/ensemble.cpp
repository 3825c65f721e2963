// ensemble.cpp — csim_ensemble_*: B single-rank members of one grid shape on one GPU, stepped together (kernels in
// ensemble.hip, device layout in ensemble.hpp).  Each member is advanced exactly as csim_stepper_run advances a
// single-rank stepper holding the same field with the same parameters, ghost ring included.
#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "ensemble.hpp"
#include "ensemble_noise.hpp"
#include "stepper.hpp"

using namespace csim;

struct csim_ensemble {
    EnsGeom g{};
    double dx = 1.0, dy = 1.0;
    double* alloc[2] = {nullptr, nullptr};
    int cur = 0;                      // alloc[cur] holds the current fields
    double* fin = nullptr;            // FinLines of every member
    void* table = nullptr;            // device: per-member entry (ens_entry_bytes() each)
    int* order = nullptr;             // device: member indices grouped by sign class
    double* scratch = nullptr;        // reduction partials
    hipStream_t st = nullptr;
    std::vector<double> D, dt, vx, vy;
    bool physics = false;             // set_physics has been called
    bool dirty = true;                // table / order need an upload
    int class_off[ENS_CLASSES + 1] = {};
    bool ring_ok = false;             // ghost rings filled and static (no Neumann side)
    int fuse = -1, fused_2c = 1, depth_used = 0;
    // per-cell statistics (csim_ensemble_stats*), created on first use: the kernel's output (mean, var, min, max),
    // its pinned host copy, and the stream that copies it while the ensemble steps on
    double* stats_d = nullptr;
    double* stats_h = nullptr;
    hipStream_t s_io = nullptr;
    hipEvent_t ev_stats = nullptr;
    bool stats_pending = false;
    // per-cell quantiles (csim_ensemble_quantiles*), the same pieces with a copy stream of their own, so that neither
    // kind of capture waits for the other's copy; the buffers grow when a call needs more fields
    double* q_d = nullptr;
    double* q_h = nullptr;
    int q_dcap = 0, q_hcap = 0;  // fields each buffer holds
    int q_nq = 0;                // levels of the capture in flight (its exceedance fields follow them in q_h)
    hipStream_t s_qio = nullptr;
    hipEvent_t ev_q = nullptr;
    bool q_pending = false;
    // verification (csim_ensemble_verify*), the same pieces again: one device buffer (histogram, per-workgroup counts
    // and sums, CRPS, Brier fields; grown to the largest call), its pinned copy, a copy stream, and a device copy of
    // a host truth with its pinned staging buffer (ev_vtruth: the staging buffer's copy has run)
    double* v_d = nullptr;
    double* v_h = nullptr;
    size_t v_dcap = 0, v_hcap = 0;  // doubles each buffer holds
    double* vtruth_d = nullptr;
    double* vtruth_h = nullptr;
    hipEvent_t ev_vtruth = nullptr;
    bool vtruth_used = false;
    hipStream_t s_vio = nullptr;
    hipEvent_t ev_v = nullptr;
    bool v_pending = false;
    int v_forecast = 0, v_nt = 0, v_blocks = 0;  // of the capture in flight
    // analysis (csim_ensemble_assimilate): one device buffer (the call's inputs in plan order and its localisation
    // table, then per-observation scalars, diagnostics and one batch's h'_k), the pinned staging buffer the inputs go
    // through, and the event after the staging buffer's last copy (ev_a).  Both buffers grow to the largest call.
    char* a_d = nullptr;
    char* a_h = nullptr;
    size_t a_dcap = 0, a_hcap = 0;  // bytes
    hipEvent_t ev_a = nullptr;
    bool a_used = false;
    // relaxation (csim_ensemble_prior_capture / csim_ensemble_relax).  A capture lives in the handle's own storage, so
    // that no call that writes the ping-pong buffers touches it: sqrt(v_b) per interior cell (RTPS), a copy of the
    // current buffer (RTPP, allocated at the first such capture), and the factor field of a call that asks for it
    double* rx_sb = nullptr;
    double* rx_prior = nullptr;
    double* rx_factor = nullptr;
    int rx_mode = 0;    // mode of the valid capture; 0: none (cleared by a run of nsteps > 0)
    int rx_truth = -1;  // its truth_member

    double* view(int buf, int m) const {
        return alloc[buf] + static_cast<size_t>(m) * g.slab + static_cast<size_t>(GHOST_EXTRA) * g.pitch;
    }
    double* base(int buf) const { return alloc[buf] + static_cast<size_t>(GHOST_EXTRA) * g.pitch; }
    bool static_ring() const {
        for (int k = 0; k < 4; ++k)
            if (g.bc[k] == CSIM_BC_NEUMANN) return false;
        return true;
    }
};

namespace {

int ensure_tables(csim_ensemble* e) {
    if (!e->dirty) return CSIM_OK;
    const int B = e->g.members;
    const size_t eb = ens_entry_bytes();
    std::vector<unsigned char> host(eb * B);
    std::vector<int> cls(B);
    for (int m = 0; m < B; ++m) {
        Phys p = make_phys(e->dx, e->dy, e->D[m], e->dt[m], e->vx[m], e->vy[m]);
        if (!e->fused_2c) p.fast_thr = 0.0;
        cls[m] = ens_sign_class(p);
        double* f = e->fin + static_cast<size_t>(m) * e->g.fin_stride;
        double* const lines[4] = {f, f + e->g.ly, f + 2 * e->g.ly, f + 2 * e->g.ly + e->g.lx};
        ens_entry_fill(host.data() + eb * m, p, lines);
    }
    std::vector<int> order;
    for (int c = 0; c < ENS_CLASSES; ++c) {
        e->class_off[c] = static_cast<int>(order.size());
        for (int m = 0; m < B; ++m)
            if (cls[m] == c) order.push_back(m);
    }
    e->class_off[ENS_CLASSES] = B;
    CSIM_HIP(hipMemcpyAsync(e->table, host.data(), eb * B, hipMemcpyHostToDevice, e->st));
    CSIM_HIP(hipMemcpyAsync(e->order, order.data(), sizeof(int) * B, hipMemcpyHostToDevice, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));  // the host vectors go out of scope
    e->dirty = false;
    return CSIM_OK;
}

size_t stats_cells(const csim_ensemble* e) { return static_cast<size_t>(e->g.nx + 2) * (e->g.ny + 2); }

// checks ddof, makes the statistics' resources, lets an in-flight copy finish (it reads stats_d), and enqueues the
// kernel on the ensemble's stream after everything enqueued so far
int stats_launch(csim_ensemble* e, int ddof) {
    CSIM_REQUIRE(ddof == 0 || ddof == 1, "ddof must be 0 or 1");
    CSIM_REQUIRE(e->g.members - ddof >= 1, "members - ddof must be >= 1");
    CSIM_REQUIRE(stats_cells(e) <= 0x7fffff00u, "grid too large for the statistics");
    const size_t bytes = 4 * sizeof(double) * stats_cells(e);
    // each piece is created once; a failed allocation is reported and retried by the next call
    if (!e->s_io) CSIM_HIP(hipStreamCreateWithFlags(&e->s_io, hipStreamNonBlocking));
    if (!e->ev_stats) CSIM_HIP(hipEventCreateWithFlags(&e->ev_stats, hipEventDisableTiming));
    if (!e->stats_d) CSIM_HIP(hipMalloc(reinterpret_cast<void**>(&e->stats_d), bytes));
    if (!e->stats_h) CSIM_HIP(hipHostMalloc(reinterpret_cast<void**>(&e->stats_h), bytes, hipHostMallocDefault));
    if (e->stats_pending) CSIM_HIP(hipStreamSynchronize(e->s_io));
    CSIM_HIP(ens_launch_stats(e->g, e->base(e->cur), ddof, e->stats_d, e->st));
    return CSIM_OK;
}

// numpy's "linear" plan of level q for n values (np.quantile; numpy/lib/_function_base_impl.py, _QuantileMethods
// ['linear'], _get_indexes, _get_gamma): v = (n - 1) q; at or past the last index both neighbours are the last one and
// gamma = v + 1 (numpy's index -1); q is in [0, 1], so v is never below 0
void quantile_plan(int n, double q, int* lo, int* hi, double* gamma) {
    const double v = static_cast<double>(n - 1) * q;
    if (v >= static_cast<double>(n - 1)) {
        *lo = *hi = n - 1;
        *gamma = v - (-1.0);
    } else {
        const double f = std::floor(v);
        *lo = static_cast<int>(f);
        *hi = *lo + 1;
        *gamma = v - f;
    }
}

int check_levels(int nq, const double* q) {
    CSIM_REQUIRE(nq >= 0 && nq <= QUANT_MAX_LEVELS, "nq must be 0 .. 16");
    CSIM_REQUIRE(nq == 0 || q, "null levels");
    for (int k = 0; k < nq; ++k) CSIM_REQUIRE(q[k] >= 0.0 && q[k] <= 1.0, "quantile levels must be in [0, 1]");  // NaN too
    return CSIM_OK;
}

// checks the arguments, makes the quantiles' resources, lets an in-flight copy finish (it reads q_d), and enqueues the
// kernel on the ensemble's stream after everything enqueued so far
int quantiles_launch(csim_ensemble* e, int nq, const double* q, int nt, const double* thr, bool pinned) {
    int rc = check_levels(nq, q);
    if (rc) return rc;
    CSIM_REQUIRE(nt >= 0 && nt <= QUANT_MAX_LEVELS, "nt must be 0 .. 16");
    CSIM_REQUIRE(nt == 0 || thr, "null thresholds");
    CSIM_REQUIRE(nq + nt >= 1, "nothing to compute: nq + nt must be >= 1");
    if (e->g.members > QUANT_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_quantiles: at most 4096 members (the largest sorting network)");
    CSIM_REQUIRE(stats_cells(e) * QUANT_MAX_LEVELS * 2 <= 0x7fffff00u, "grid too large for the quantiles");
    QuantArgs qa{};
    qa.nq = nq;
    qa.nt = nt;
    for (int k = 0; k < nq; ++k) quantile_plan(e->g.members, q[k], &qa.lo[k], &qa.hi[k], &qa.g[k]);
    for (int k = 0; k < nt; ++k) qa.thr[k] = thr[k];

    if (!e->s_qio) CSIM_HIP(hipStreamCreateWithFlags(&e->s_qio, hipStreamNonBlocking));
    if (!e->ev_q) CSIM_HIP(hipEventCreateWithFlags(&e->ev_q, hipEventDisableTiming));
    if (e->q_pending) CSIM_HIP(hipStreamSynchronize(e->s_qio));
    // grow a buffer that is too small for this call: nothing reads q_d or q_h once the copy above and the kernels
    // enqueued so far are done; a failed allocation leaves the buffer absent, and the next call tries again
    const int fields = nq + nt;
    const size_t bytes = sizeof(double) * fields * stats_cells(e);
    if (fields > e->q_dcap) {
        CSIM_HIP(hipStreamSynchronize(e->st));
        if (e->q_d) (void)hipFree(e->q_d);
        e->q_d = nullptr;
        e->q_dcap = 0;
        CSIM_HIP(hipMalloc(reinterpret_cast<void**>(&e->q_d), bytes));
        e->q_dcap = fields;
    }
    if (pinned && fields > e->q_hcap) {
        if (e->q_h) (void)hipHostFree(e->q_h);
        e->q_h = nullptr;
        e->q_hcap = 0;
        e->q_pending = false;
        CSIM_HIP(hipHostMalloc(reinterpret_cast<void**>(&e->q_h), bytes, hipHostMallocDefault));
        e->q_hcap = fields;
    }
    CSIM_HIP(ens_launch_quantiles(e->g, e->base(e->cur), qa, e->q_d, e->st));
    return CSIM_OK;
}

// the verification buffer, in doubles: rank histogram (M + 1), counts (2 per workgroup), sums (VERIFY_SUMS per
// workgroup), CRPS, nt Brier fields
struct VerifyLayout {
    size_t hist, counts, sums, crps, brier, total;
};
VerifyLayout verify_layout(int forecast, int blocks, int nt, size_t cells) {
    VerifyLayout l{};
    l.hist = 0;
    l.counts = l.hist + forecast + 1;
    l.sums = l.counts + 2 * static_cast<size_t>(blocks);
    l.crps = l.sums + static_cast<size_t>(VERIFY_SUMS) * blocks;
    l.brier = l.crps + cells;
    l.total = l.brier + static_cast<size_t>(nt) * cells;
    return l;
}

// the domain scores from the per-workgroup records, added in workgroup order
void verify_finish(const unsigned long long* counts, const double* sums, int blocks, int nt, csim_verify_scores* s) {
    long long n = 0, nan = 0;
    for (int b = 0; b < blocks; ++b) {
        n += static_cast<long long>(counts[2 * b]);
        nan += static_cast<long long>(counts[2 * b + 1]);
    }
    double tot[VERIFY_SUMS] = {};
    for (int q = 0; q < 3 + nt; ++q) {
        double acc = sums[q];
        for (int b = 1; b < blocks; ++b) acc += sums[static_cast<size_t>(b) * VERIFY_SUMS + q];
        tot[q] = acc;
    }
    const double cells = static_cast<double>(n), nanv = std::nan("");
    std::memset(s, 0, sizeof(*s));
    s->cells = n;
    s->nan_cells = nan;
    s->crps = n ? tot[0] / cells : nanv;
    s->rmse = n ? std::sqrt(tot[1] / cells) : nanv;
    s->spread = n ? std::sqrt(tot[2] / cells) : nanv;
    for (int k = 0; k < nt; ++k) s->brier[k] = n ? tot[3 + k] / cells : nanv;
}

// checks the arguments, makes the verification's resources, lets an in-flight copy finish (it reads v_d), stages a
// host truth, and enqueues the histogram's zeroing and the kernel on the ensemble's stream after everything enqueued
// so far.  *forecast, *blocks: of this call
int verify_launch(csim_ensemble* e, const double* truth, int truth_member, int fair, int nt, const double* thr,
                  bool pinned, int* forecast, int* blocks) {
    const int B = e->g.members;
    CSIM_REQUIRE((truth != nullptr) != (truth_member >= 0), "give exactly one truth: a host field or a member");
    CSIM_REQUIRE(truth_member >= -1 && truth_member < B, "truth_member out of range");
    CSIM_REQUIRE(nt >= 0 && nt <= VERIFY_MAX_THRESHOLDS, "nt must be 0 .. 16");
    CSIM_REQUIRE(nt == 0 || thr, "null thresholds");
    CSIM_REQUIRE(fair == 0 || fair == 1, "fair must be 0 or 1");
    const int M = truth ? B : B - 1;
    CSIM_REQUIRE(M >= 1, "no forecast members: a truth member needs at least two members");
    CSIM_REQUIRE(!fair || M >= 2, "the fair CRPS needs at least two forecast members");
    if (M > VERIFY_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_verify: at most 4096 forecast members (the largest sorting network)");
    CSIM_REQUIRE(stats_cells(e) * (VERIFY_MAX_THRESHOLDS + 1) <= 0x7fffff00u, "grid too large for the verification");
    const size_t cells = stats_cells(e);
    const int nb = ens_verify_blocks(e->g, M);
    const VerifyLayout l = verify_layout(M, nb, nt, cells);

    if (!e->s_vio) CSIM_HIP(hipStreamCreateWithFlags(&e->s_vio, hipStreamNonBlocking));
    if (!e->ev_v) CSIM_HIP(hipEventCreateWithFlags(&e->ev_v, hipEventDisableTiming));
    if (!e->ev_vtruth) CSIM_HIP(hipEventCreateWithFlags(&e->ev_vtruth, hipEventDisableTiming));
    if (e->v_pending) CSIM_HIP(hipStreamSynchronize(e->s_vio));
    // grow a buffer that is too small for this call (as quantiles_launch does)
    if (l.total > e->v_dcap) {
        CSIM_HIP(hipStreamSynchronize(e->st));
        if (e->v_d) (void)hipFree(e->v_d);
        e->v_d = nullptr;
        e->v_dcap = 0;
        CSIM_HIP(hipMalloc(reinterpret_cast<void**>(&e->v_d), sizeof(double) * l.total));
        e->v_dcap = l.total;
    }
    if (pinned && l.total > e->v_hcap) {
        if (e->v_h) (void)hipHostFree(e->v_h);
        e->v_h = nullptr;
        e->v_hcap = 0;
        e->v_pending = false;
        CSIM_HIP(hipHostMalloc(reinterpret_cast<void**>(&e->v_h), sizeof(double) * l.total, hipHostMallocDefault));
        e->v_hcap = l.total;
    }
    VerifyArgs va{};
    va.forecast = M;
    va.truth_member = truth ? B : truth_member;
    va.nt = nt;
    va.fair = fair;
    for (int k = 0; k < nt; ++k) va.thr[k] = thr[k];
    if (truth) {  // copied before the call returns: host -> pinned staging -> device, in stream order
        if (!e->vtruth_d) CSIM_HIP(hipMalloc(reinterpret_cast<void**>(&e->vtruth_d), sizeof(double) * cells));
        if (!e->vtruth_h)
            CSIM_HIP(hipHostMalloc(reinterpret_cast<void**>(&e->vtruth_h), sizeof(double) * cells, hipHostMallocDefault));
        if (e->vtruth_used) CSIM_HIP(hipEventSynchronize(e->ev_vtruth));  // the staging buffer's last copy is done
        std::memcpy(e->vtruth_h, truth, sizeof(double) * cells);
        CSIM_HIP(hipMemcpyAsync(e->vtruth_d, e->vtruth_h, sizeof(double) * cells, hipMemcpyHostToDevice, e->st));
        CSIM_HIP(hipEventRecord(e->ev_vtruth, e->st));
        e->vtruth_used = true;
        va.truth = e->vtruth_d;
    }
    VerifyOut o{};
    o.hist = reinterpret_cast<unsigned long long*>(e->v_d + l.hist);
    o.counts = reinterpret_cast<unsigned long long*>(e->v_d + l.counts);
    o.sums = e->v_d + l.sums;
    o.crps = e->v_d + l.crps;
    o.brier = e->v_d + l.brier;
    CSIM_HIP(hipMemsetAsync(o.hist, 0, sizeof(unsigned long long) * (M + 1), e->st));
    CSIM_HIP(ens_launch_verify(e->g, e->base(e->cur), va, o, e->st));
    *forecast = M;
    *blocks = nb;
    return CSIM_OK;
}

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

constexpr size_t ASSIM_HP_DOUBLES = size_t(1) << 23;  // h'_k of one batch: 64 MiB, at least 8192 observations

// the checks csim_ensemble_prior_capture and csim_ensemble_relax share; *forecast = M
int relax_check(const csim_ensemble* e, int mode, int truth_member, int* forecast) {
    const int B = e->g.members;
    CSIM_REQUIRE(mode == CSIM_RELAX_SPREAD || mode == CSIM_RELAX_PERT, "mode must be CSIM_RELAX_SPREAD or CSIM_RELAX_PERT");
    CSIM_REQUIRE(truth_member >= -1 && truth_member < B, "truth_member out of range");
    const int M = truth_member >= 0 ? B - 1 : B;
    CSIM_REQUIRE(M >= 2, "the relaxation needs at least two forecast members");
    if (M > ASSIM_MAX_MEMBERS) return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_relax: at most 1024 forecast members");
    CSIM_REQUIRE(e->g.slab <= 0x7fffffffL, "grid too large for the relaxation");
    *forecast = M;
    return CSIM_OK;
}

int ghost_fill(csim_ensemble* e, bool fin) {
    CSIM_HIP(ens_launch_ghost_fill(e->g, e->base(e->cur), e->base(1 - e->cur), e->table, fin, e->st));
    return CSIM_OK;
}

}  // namespace

extern "C" {

int csim_ensemble_plan(int nsteps, int nx, int ny, int fuse, int out[3]) {
    CSIM_REQUIRE(out && nsteps >= 0 && nx >= 1 && ny >= 1, "bad argument");
    CSIM_REQUIRE(fuse >= -1 && fuse <= 1, "fuse must be -1 (auto), 0 or 1");
    const int T = (fuse < 0 && nx >= ENS_DEPTH && ny >= ENS_DEPTH) ? ENS_DEPTH : 1;
    out[0] = T;
    out[1] = T > 1 ? nsteps / T : 0;
    out[2] = T > 1 ? nsteps % T : nsteps;
    return CSIM_OK;
}

int csim_ensemble_sign_class(double dx, double dy, double D, double dt, double vx, double vy, int fused_2c, int* cls) {
    CSIM_REQUIRE(cls && dx > 0 && dy > 0, "bad argument");
    Phys p = make_phys(dx, dy, D, dt, vx, vy);
    if (!fused_2c) p.fast_thr = 0.0;
    *cls = ens_sign_class(p);
    return CSIM_OK;
}

int csim_ensemble_classes(int members, const int* cls, int* nlaunches) {
    CSIM_REQUIRE(members >= 1 && cls && nlaunches, "bad argument");
    bool seen[ENS_CLASSES] = {};
    int n = 0;
    for (int m = 0; m < members; ++m) {
        CSIM_REQUIRE(cls[m] >= 0 && cls[m] < ENS_CLASSES, "sign class out of range");
        if (!seen[cls[m]]) ++n;
        seen[cls[m]] = true;
    }
    *nlaunches = n;
    return CSIM_OK;
}

int csim_ensemble_create(int members, int nx, int ny, int halo, double dx, double dy, const int bc[4],
                         double bc_value, csim_ensemble** out) {
    CSIM_REQUIRE(out, "out is null");
    *out = nullptr;
    CSIM_REQUIRE(bc, "null argument");
    CSIM_REQUIRE(members >= 1 && members <= 65535, "members must be 1 .. 65535");
    CSIM_REQUIRE(nx >= 1 && ny >= 1, "empty grid");
    CSIM_REQUIRE(halo == 1, "only halo == 1 is supported");
    CSIM_REQUIRE(dx > 0 && dy > 0 && std::isfinite(dx) && std::isfinite(dy), "dx/dy must be finite and > 0");
    for (int k = 0; k < 4; ++k)
        CSIM_REQUIRE(bc[k] >= CSIM_BC_DIRICHLET && bc[k] <= CSIM_BC_PERIODIC, "unknown boundary type");
    csim_ensemble* e = new csim_ensemble;
    EnsGeom& g = e->g;
    g.members = members, g.nx = nx, g.ny = ny, g.pitch = pitch_for(nx);
    g.slab = static_cast<long>(ny + 2 + 2 * GHOST_EXTRA) * g.pitch;
    g.lx = round_up(nx, 2), g.ly = round_up(ny, 2);
    g.fin_stride = 2L * g.lx + 2L * g.ly;
    for (int k = 0; k < 4; ++k) g.bc[k] = bc[k];
    g.value = bc_value;
    e->dx = dx, e->dy = dy;
    g.div_mode = make_phys(dx, dy, 0.0, 0.0, 0.0, 0.0).div_mode;
    e->D.assign(members, 0.0), e->dt.assign(members, 0.0), e->vx.assign(members, 0.0), e->vy.assign(members, 0.0);
    const size_t bytes = sizeof(double) * static_cast<size_t>(g.slab) * members;
    const size_t nred = static_cast<size_t>(members) * 2 * ENS_REDUCE_ROWS;
    hipError_t err = hipSuccess;
    auto ok = [&](hipError_t r) {
        if (err == hipSuccess) err = r;
        return err == hipSuccess;
    };
    // zero-filled: the pads and the device-only ghost layers the multi-step sweep reads as don't-care must be finite
    ok(hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking)) && ok(hipMalloc(&e->alloc[0], bytes)) &&
        ok(hipMalloc(&e->alloc[1], bytes)) && ok(hipMemset(e->alloc[0], 0, bytes)) && ok(hipMemset(e->alloc[1], 0, bytes)) &&
        ok(hipMalloc(&e->fin, sizeof(double) * g.fin_stride * members)) &&
        ok(hipMemset(e->fin, 0, sizeof(double) * g.fin_stride * members)) &&
        ok(hipMalloc(&e->table, ens_entry_bytes() * members)) && ok(hipMalloc(&e->order, sizeof(int) * members)) &&
        ok(hipMalloc(&e->scratch, sizeof(double) * nred));
    if (err != hipSuccess) {
        csim_ensemble_destroy(e);
        return fail(CSIM_ERR_HIP, std::string("csim_ensemble_create: ") + hipGetErrorString(err));
    }
    *out = e;
    return CSIM_OK;
}

int csim_ensemble_destroy(csim_ensemble* e) {
    if (!e) return CSIM_OK;
    if (e->st) (void)hipStreamSynchronize(e->st);
    if (e->s_io) (void)hipStreamSynchronize(e->s_io);
    if (e->stats_d) (void)hipFree(e->stats_d);
    if (e->stats_h) (void)hipHostFree(e->stats_h);
    if (e->ev_stats) (void)hipEventDestroy(e->ev_stats);
    if (e->s_io) (void)hipStreamDestroy(e->s_io);
    if (e->s_qio) (void)hipStreamSynchronize(e->s_qio);
    if (e->q_d) (void)hipFree(e->q_d);
    if (e->q_h) (void)hipHostFree(e->q_h);
    if (e->ev_q) (void)hipEventDestroy(e->ev_q);
    if (e->s_qio) (void)hipStreamDestroy(e->s_qio);
    if (e->s_vio) (void)hipStreamSynchronize(e->s_vio);
    if (e->v_d) (void)hipFree(e->v_d);
    if (e->v_h) (void)hipHostFree(e->v_h);
    if (e->vtruth_d) (void)hipFree(e->vtruth_d);
    if (e->vtruth_h) (void)hipHostFree(e->vtruth_h);
    if (e->ev_vtruth) (void)hipEventDestroy(e->ev_vtruth);
    if (e->ev_v) (void)hipEventDestroy(e->ev_v);
    if (e->s_vio) (void)hipStreamDestroy(e->s_vio);
    if (e->a_d) (void)hipFree(e->a_d);
    if (e->a_h) (void)hipHostFree(e->a_h);
    if (e->ev_a) (void)hipEventDestroy(e->ev_a);
    if (e->rx_sb) (void)hipFree(e->rx_sb);
    if (e->rx_prior) (void)hipFree(e->rx_prior);
    if (e->rx_factor) (void)hipFree(e->rx_factor);
    for (double* a : e->alloc)
        if (a) (void)hipFree(a);
    if (e->fin) (void)hipFree(e->fin);
    if (e->table) (void)hipFree(e->table);
    if (e->order) (void)hipFree(e->order);
    if (e->scratch) (void)hipFree(e->scratch);
    if (e->st) (void)hipStreamDestroy(e->st);
    delete e;
    return CSIM_OK;
}

int csim_ensemble_upload(csim_ensemble* e, int member, const double* host_with_ghosts) {
    CSIM_REQUIRE(e && host_with_ghosts, "null argument");
    CSIM_REQUIRE(member >= 0 && member < e->g.members, "member out of range");
    CSIM_HIP(hipStreamSynchronize(e->st));
    // both ping-pong buffers get the field: they start with the same ghost ring (reference main.cpp:104 copies u->tmp),
    // which periodic sides keep for good
    int rc = upload_2d(e->view(e->cur, member), e->g.nx, e->g.ny, e->g.pitch, host_with_ghosts);
    if (!rc) rc = upload_2d(e->view(1 - e->cur, member), e->g.nx, e->g.ny, e->g.pitch, host_with_ghosts);
    e->ring_ok = false;
    return rc;
}

int csim_ensemble_upload_all(csim_ensemble* e, const double* host) {
    CSIM_REQUIRE(e && host, "null argument");
    const size_t per = static_cast<size_t>(e->g.nx + 2) * (e->g.ny + 2);
    for (int m = 0; m < e->g.members; ++m) {
        int rc = csim_ensemble_upload(e, m, host + per * m);
        if (rc) return rc;
    }
    return CSIM_OK;
}

int csim_ensemble_download(csim_ensemble* e, int member, double* host_with_ghosts) {
    CSIM_REQUIRE(e && host_with_ghosts, "null argument");
    CSIM_REQUIRE(member >= 0 && member < e->g.members, "member out of range");
    CSIM_HIP(hipStreamSynchronize(e->st));
    return download_2d(e->view(e->cur, member), e->g.nx, e->g.ny, e->g.pitch, host_with_ghosts);
}

int csim_ensemble_download_all(csim_ensemble* e, double* host) {
    CSIM_REQUIRE(e && host, "null argument");
    const size_t per = static_cast<size_t>(e->g.nx + 2) * (e->g.ny + 2);
    for (int m = 0; m < e->g.members; ++m) {
        int rc = csim_ensemble_download(e, m, host + per * m);
        if (rc) return rc;
    }
    return CSIM_OK;
}

int csim_ensemble_init_gaussian(csim_ensemble* e, int member, double A, double sigma_frac, double xc_frac,
                                double yc_frac) {
    CSIM_REQUIRE(e, "null argument");
    CSIM_REQUIRE(member >= 0 && member < e->g.members, "member out of range");
    // as csim_stepper_init_gaussian: the member's whole slab (ghost ring included) zeroed, the hotspot written, and
    // the same slab in the other buffer
    const size_t slab = sizeof(double) * static_cast<size_t>(e->g.slab);
    double* cur = e->alloc[e->cur] + static_cast<size_t>(member) * e->g.slab;
    double* other = e->alloc[1 - e->cur] + static_cast<size_t>(member) * e->g.slab;
    CSIM_HIP(hipMemsetAsync(cur, 0, slab, e->st));
    CSIM_HIP(launch_gaussian(e->view(e->cur, member), e->g.nx, e->g.ny, e->g.pitch, 0, 0, e->g.nx, e->g.ny, e->dx,
                             e->dy, A, sigma_frac, xc_frac, yc_frac, e->st));
    CSIM_HIP(hipMemcpyAsync(other, cur, slab, hipMemcpyDeviceToDevice, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    e->ring_ok = false;
    return CSIM_OK;
}

int csim_ensemble_set_physics(csim_ensemble* e, const double* D, const double* dt, const double* vx, const double* vy) {
    CSIM_REQUIRE(e && D && dt && vx && vy, "null argument");
    for (int m = 0; m < e->g.members; ++m)
        CSIM_REQUIRE(std::isfinite(dt[m]), "dt must be finite");
    e->D.assign(D, D + e->g.members);
    e->dt.assign(dt, dt + e->g.members);
    e->vx.assign(vx, vx + e->g.members);
    e->vy.assign(vy, vy + e->g.members);
    e->physics = true;
    e->dirty = true;
    return CSIM_OK;
}

int csim_ensemble_run(csim_ensemble* e, int nsteps) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_REQUIRE(nsteps >= 0, "nsteps must be >= 0");
    if (!e->physics) return fail(CSIM_ERR_STATE, "csim_ensemble_set_physics first");
    int plan[3];
    int rc = csim_ensemble_plan(nsteps, e->g.nx, e->g.ny, e->fuse, plan);
    if (rc) return rc;
    rc = ensure_tables(e);
    if (rc) return rc;
    const int q = plan[1], r = plan[2];
    const bool stat = e->static_ring();
    if (nsteps > 0) e->rx_mode = 0;  // the forecast a relaxation capture was taken of is gone
    // q passes of ENS_DEPTH steps, one launch per sign class present; the last one of the run leaves the FinLines
    // (unless the ring is static) from which the closing ghost fill makes the reference's ring
    for (int k = 0; k < q; ++k) {
        if (!e->ring_ok) {
            rc = ghost_fill(e, false);
            if (rc) return rc;
            e->ring_ok = stat;
        }
        const bool final_pass = k == q - 1 && r == 0 && !e->ring_ok;
        for (int c = 0; c < ENS_CLASSES; ++c) {
            const int n = e->class_off[c + 1] - e->class_off[c];
            if (n == 0) continue;
            CSIM_HIP(ens_launch_sweepO(e->g, e->base(e->cur), e->base(1 - e->cur), e->table, e->order + e->class_off[c],
                                       n, c, final_pass, e->st));
        }
        e->cur = 1 - e->cur;
        if (final_pass) {
            rc = ghost_fill(e, true);
            if (rc) return rc;
        }
    }
    for (int k = 0; k < r; ++k) {
        if (!e->ring_ok) {
            rc = ghost_fill(e, false);
            if (rc) return rc;
            e->ring_ok = stat;
        }
        CSIM_HIP(ens_launch_step(e->g, e->base(e->cur), e->base(1 - e->cur), e->table, e->st));
        e->cur = 1 - e->cur;
    }
    if (nsteps > 0) e->depth_used = q > 0 ? plan[0] : 1;  // a run shorter than one pass takes single steps only
    return CSIM_OK;
}

int csim_ensemble_sync(csim_ensemble* e) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_HIP(hipStreamSynchronize(e->st));
    return CSIM_OK;
}

int csim_ensemble_checksum(csim_ensemble* e, unsigned long long* out) {
    CSIM_REQUIRE(e && out, "null argument");
    const int R = ens_reduce_rows(e->g.ny), B = e->g.members;
    auto* part = reinterpret_cast<unsigned long long*>(e->scratch);
    CSIM_HIP(ens_launch_checksum(e->g, e->base(e->cur), part, e->st));
    std::vector<unsigned long long> h(static_cast<size_t>(R) * B);
    CSIM_HIP(hipMemcpyAsync(h.data(), part, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    for (int m = 0; m < B; ++m) {
        unsigned long long acc = 0;
        for (int k = 0; k < R; ++k) acc += h[static_cast<size_t>(m) * R + k];
        out[m] = acc;
    }
    return CSIM_OK;
}

int csim_ensemble_minmax(csim_ensemble* e, double* out) {
    CSIM_REQUIRE(e && out, "null argument");
    const int R = ens_reduce_rows(e->g.ny + 2), B = e->g.members;
    CSIM_HIP(ens_launch_minmax(e->g, e->base(e->cur), e->scratch, e->st));
    std::vector<double> h(2 * static_cast<size_t>(R) * B);
    CSIM_HIP(hipMemcpyAsync(h.data(), e->scratch, sizeof(double) * h.size(), hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    const size_t hi = static_cast<size_t>(R) * B;
    for (int m = 0; m < B; ++m) {
        const size_t k0 = static_cast<size_t>(m) * R;
        double lo = h[k0], up = h[hi + k0];
        for (int k = 1; k < R; ++k) {
            lo = std::fmin(lo, h[k0 + k]);
            up = std::fmax(up, h[hi + k0 + k]);
        }
        out[2 * m] = lo;
        out[2 * m + 1] = up;
    }
    return CSIM_OK;
}

int csim_ensemble_sum(csim_ensemble* e, double* out) {
    CSIM_REQUIRE(e && out, "null argument");
    const int R = ens_reduce_rows(e->g.ny), B = e->g.members;
    CSIM_HIP(ens_launch_sum(e->g, e->base(e->cur), e->scratch, e->st));
    std::vector<double> h(static_cast<size_t>(R) * B);
    CSIM_HIP(hipMemcpyAsync(h.data(), e->scratch, sizeof(double) * h.size(), hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    for (int m = 0; m < B; ++m) {
        double acc = h[static_cast<size_t>(m) * R];
        for (int k = 1; k < R; ++k) acc += h[static_cast<size_t>(m) * R + k];
        out[m] = acc;
    }
    return CSIM_OK;
}

int csim_ensemble_stats(csim_ensemble* e, int ddof, double* mean, double* var, double* min, double* max) {
    CSIM_REQUIRE(e, "null ensemble");
    int rc = stats_launch(e, ddof);
    if (rc) return rc;
    const size_t n = stats_cells(e);
    double* const outs[4] = {mean, var, min, max};
    for (int k = 0; k < 4; ++k)
        if (outs[k])
            CSIM_HIP(hipMemcpyAsync(outs[k], e->stats_d + k * n, sizeof(double) * n, hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    return CSIM_OK;
}

// As csim_stepper_snapshot_begin: the kernel runs in stream order on the ensemble's stream (the sweeps after it write
// the other buffer first, and never stats_d), and only the copy to the pinned buffer goes to s_io, so the next run
// does not wait for it.
int csim_ensemble_stats_begin(csim_ensemble* e, int ddof) {
    CSIM_REQUIRE(e, "null ensemble");
    int rc = stats_launch(e, ddof);
    if (rc) return rc;
    CSIM_HIP(hipEventRecord(e->ev_stats, e->st));
    CSIM_HIP(hipStreamWaitEvent(e->s_io, e->ev_stats, 0));
    CSIM_HIP(hipMemcpyAsync(e->stats_h, e->stats_d, 4 * sizeof(double) * stats_cells(e), hipMemcpyDeviceToHost,
                            e->s_io));
    e->stats_pending = true;
    return CSIM_OK;
}

int csim_ensemble_stats_wait(csim_ensemble* e, const double** mean, const double** var, const double** min,
                             const double** max) {
    CSIM_REQUIRE(e, "null ensemble");
    if (!e->stats_pending) return fail(CSIM_ERR_STATE, "no statistics in flight: csim_ensemble_stats_begin first");
    CSIM_HIP(hipStreamSynchronize(e->s_io));
    e->stats_pending = false;
    const double** const outs[4] = {mean, var, min, max};
    for (int k = 0; k < 4; ++k)
        if (outs[k]) *outs[k] = e->stats_h + k * stats_cells(e);
    return CSIM_OK;
}

int csim_ensemble_quantiles(csim_ensemble* e, int nq, const double* q, int nt, const double* thr, double* out_q,
                            double* out_p) {
    CSIM_REQUIRE(e, "null ensemble");
    int rc = quantiles_launch(e, nq, q, nt, thr, false);
    if (rc) return rc;
    const size_t n = stats_cells(e);
    if (out_q && nq)
        CSIM_HIP(hipMemcpyAsync(out_q, e->q_d, sizeof(double) * nq * n, hipMemcpyDeviceToHost, e->st));
    if (out_p && nt)
        CSIM_HIP(hipMemcpyAsync(out_p, e->q_d + nq * n, sizeof(double) * nt * n, hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    return CSIM_OK;
}

// As csim_ensemble_stats_begin, with the copy on s_qio
int csim_ensemble_quantiles_begin(csim_ensemble* e, int nq, const double* q, int nt, const double* thr) {
    CSIM_REQUIRE(e, "null ensemble");
    int rc = quantiles_launch(e, nq, q, nt, thr, true);
    if (rc) return rc;
    CSIM_HIP(hipEventRecord(e->ev_q, e->st));
    CSIM_HIP(hipStreamWaitEvent(e->s_qio, e->ev_q, 0));
    CSIM_HIP(hipMemcpyAsync(e->q_h, e->q_d, sizeof(double) * (nq + nt) * stats_cells(e), hipMemcpyDeviceToHost,
                            e->s_qio));
    e->q_nq = nq;
    e->q_pending = true;
    return CSIM_OK;
}

int csim_ensemble_quantiles_wait(csim_ensemble* e, const double** out_q, const double** out_p) {
    CSIM_REQUIRE(e, "null ensemble");
    if (!e->q_pending) return fail(CSIM_ERR_STATE, "no quantiles in flight: csim_ensemble_quantiles_begin first");
    CSIM_HIP(hipStreamSynchronize(e->s_qio));
    e->q_pending = false;
    if (out_q) *out_q = e->q_h;
    if (out_p) *out_p = e->q_h + e->q_nq * stats_cells(e);
    return CSIM_OK;
}

int csim_ensemble_quantile_plan(int members, int nq, const double* q, int* lo, int* hi, double* gamma) {
    CSIM_REQUIRE(members >= 1, "members must be >= 1");
    int rc = check_levels(nq, q);
    if (rc) return rc;
    CSIM_REQUIRE(nq == 0 || (lo && hi && gamma), "null output");
    for (int k = 0; k < nq; ++k) quantile_plan(members, q[k], &lo[k], &hi[k], &gamma[k]);
    return CSIM_OK;
}

int csim_ensemble_verify(csim_ensemble* e, const double* truth, int truth_member, int fair, int nt, const double* thr,
                         double* out_crps, double* out_brier, unsigned long long* rank_hist,
                         csim_verify_scores* scores) {
    CSIM_REQUIRE(e, "null ensemble");
    int M = 0, nb = 0;
    int rc = verify_launch(e, truth, truth_member, fair, nt, thr, false, &M, &nb);
    if (rc) return rc;
    const size_t cells = stats_cells(e);
    const VerifyLayout l = verify_layout(M, nb, nt, cells);
    std::vector<double> rec;
    if (out_crps)
        CSIM_HIP(hipMemcpyAsync(out_crps, e->v_d + l.crps, sizeof(double) * cells, hipMemcpyDeviceToHost, e->st));
    if (out_brier && nt)
        CSIM_HIP(hipMemcpyAsync(out_brier, e->v_d + l.brier, sizeof(double) * nt * cells, hipMemcpyDeviceToHost, e->st));
    if (rank_hist)
        CSIM_HIP(hipMemcpyAsync(rank_hist, e->v_d + l.hist, sizeof(unsigned long long) * (M + 1), hipMemcpyDeviceToHost,
                                e->st));
    if (scores) {
        rec.resize(l.crps - l.counts);
        CSIM_HIP(hipMemcpyAsync(rec.data(), e->v_d + l.counts, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, e->st));
    }
    CSIM_HIP(hipStreamSynchronize(e->st));
    if (scores)
        verify_finish(reinterpret_cast<const unsigned long long*>(rec.data()), rec.data() + (l.sums - l.counts), nb, nt,
                      scores);
    return CSIM_OK;
}

// As csim_ensemble_quantiles_begin, with the copy on s_vio; the scores are finished in _wait
int csim_ensemble_verify_begin(csim_ensemble* e, const double* truth, int truth_member, int fair, int nt,
                               const double* thr) {
    CSIM_REQUIRE(e, "null ensemble");
    int M = 0, nb = 0;
    int rc = verify_launch(e, truth, truth_member, fair, nt, thr, true, &M, &nb);
    if (rc) return rc;
    const VerifyLayout l = verify_layout(M, nb, nt, stats_cells(e));
    CSIM_HIP(hipEventRecord(e->ev_v, e->st));
    CSIM_HIP(hipStreamWaitEvent(e->s_vio, e->ev_v, 0));
    CSIM_HIP(hipMemcpyAsync(e->v_h, e->v_d, sizeof(double) * l.total, hipMemcpyDeviceToHost, e->s_vio));
    e->v_forecast = M;
    e->v_nt = nt;
    e->v_blocks = nb;
    e->v_pending = true;
    return CSIM_OK;
}

int csim_ensemble_verify_wait(csim_ensemble* e, const double** out_crps, const double** out_brier,
                              const unsigned long long** rank_hist, csim_verify_scores* scores) {
    CSIM_REQUIRE(e, "null ensemble");
    if (!e->v_pending) return fail(CSIM_ERR_STATE, "no verification in flight: csim_ensemble_verify_begin first");
    CSIM_HIP(hipStreamSynchronize(e->s_vio));
    e->v_pending = false;
    const VerifyLayout l = verify_layout(e->v_forecast, e->v_blocks, e->v_nt, stats_cells(e));
    if (out_crps) *out_crps = e->v_h + l.crps;
    if (out_brier) *out_brier = e->v_h + l.brier;
    if (rank_hist) *rank_hist = reinterpret_cast<const unsigned long long*>(e->v_h + l.hist);
    if (scores)
        verify_finish(reinterpret_cast<const unsigned long long*>(e->v_h + l.counts), e->v_h + l.sums, e->v_blocks,
                      e->v_nt, scores);
    return CSIM_OK;
}

int csim_ensemble_rank_slot(long long g, int ties, int* slot) {
    CSIM_REQUIRE(slot && g >= 0 && ties >= 0, "bad argument");
    *slot = static_cast<int>(verify_mix(static_cast<unsigned long long>(g)) % (static_cast<unsigned long long>(ties) + 1));
    return CSIM_OK;
}

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
    CSIM_REQUIRE(truth_member >= -1 && truth_member < B, "truth_member out of range");
    CSIM_REQUIRE(ordered == 0 || ordered == 1, "ordered must be 0 or 1");
    const int M = truth_member >= 0 ? B - 1 : B;
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
    int rc = csim_ensemble_gc_table(e->dx, e->dy, loc, g.nx, g.ny, &lx, &ly, nullptr);
    if (rc) return rc;
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
    const int batch = static_cast<int>(std::min<size_t>(ASSIM_HP_DOUBLES / M, ASSIM_MAX_OBS));
    const size_t hp = static_cast<size_t>(std::min(nobs, batch)) * M;
    const AssimLayout l = assim_layout(nobs, tcells, hp);

    // resources: the device buffer grows after the work already enqueued is done with it, the staging buffer after
    // its last copy has run
    if (!e->ev_a) CSIM_HIP(hipEventCreateWithFlags(&e->ev_a, hipEventDisableTiming));
    if (l.total > e->a_dcap) {
        CSIM_HIP(hipStreamSynchronize(e->st));
        if (e->a_d) (void)hipFree(e->a_d);
        e->a_d = nullptr;
        e->a_dcap = 0;
        CSIM_HIP(hipMalloc(reinterpret_cast<void**>(&e->a_d), l.total));
        e->a_dcap = l.total;
    }
    if (e->a_used) CSIM_HIP(hipEventSynchronize(e->ev_a));
    e->a_used = false;
    if (l.staged > e->a_hcap) {
        if (e->a_h) (void)hipHostFree(e->a_h);
        e->a_h = nullptr;
        e->a_hcap = 0;
        CSIM_HIP(hipHostMalloc(reinterpret_cast<void**>(&e->a_h), l.staged, hipHostMallocDefault));
        e->a_hcap = l.staged;
    }
    char* h = e->a_h;
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
    CSIM_HIP(hipMemcpyAsync(e->a_d, h, l.staged, hipMemcpyHostToDevice, e->st));
    CSIM_HIP(hipEventRecord(e->ev_a, e->st));
    e->a_used = true;

    AssimArgs a{};
    a.forecast = M;
    a.truth_member = truth_member >= 0 ? truth_member : B;
    a.lx = lx, a.ly = ly;
    a.rho = reinterpret_cast<const double*>(e->a_d + l.rho);
    a.obs.i = reinterpret_cast<const int*>(e->a_d + l.i);
    a.obs.j = reinterpret_cast<const int*>(e->a_d + l.j);
    a.obs.idx = reinterpret_cast<const int*>(e->a_d + l.idx);
    a.obs.y = reinterpret_cast<const double*>(e->a_d + l.y);
    a.obs.r = reinterpret_cast<const double*>(e->a_d + l.r);
    a.scal = reinterpret_cast<double*>(e->a_d + l.scal);
    a.hp = reinterpret_cast<double*>(e->a_d + l.hp);
    a.prior = prior_mean || prior_var ? reinterpret_cast<double*>(e->a_d + l.prior) : nullptr;
    double* f = e->base(e->cur);
    if (inflation != 1.0) CSIM_HIP(ens_launch_assim_inflate(g, f, M, a.truth_member, inflation - 1.0, e->st));
    for (int L = 0; L < nl; ++L)
        for (int q0 = off[L]; q0 < off[L + 1]; q0 += batch) {
            const int n = std::min(batch, off[L + 1] - q0);
            long wcells = 0;
            for (int q = q0; q < q0 + n; ++q) {
                const long w = std::min(g.nx, hi[q] + lx) - std::max(1, hi[q] - lx) + 1;
                const long hgt = std::min(g.ny, hj[q] + ly) - std::max(1, hj[q] - ly) + 1;
                wcells = std::max(wcells, w * hgt);
            }
            CSIM_HIP(ens_launch_assim_prior(g, f, a, q0, n, e->st));
            CSIM_HIP(ens_launch_assim_update(g, f, a, q0, n, wcells, e->st));
        }
    if (!diag) return CSIM_OK;
    auto* post = reinterpret_cast<double*>(e->a_d + l.post);
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
    CSIM_REQUIRE(truth_member >= -1 && truth_member < B, "truth_member out of range");
    const int M = truth_member >= 0 ? B - 1 : B;
    CSIM_REQUIRE(M >= 1, "no forecast member");
    CSIM_REQUIRE(!centered || M >= 2, "centering needs at least two forecast members");
    PerturbArgs a{};
    a.perx = g.bc[CSIM_LEFT] == CSIM_BC_PERIODIC && g.bc[CSIM_RIGHT] == CSIM_BC_PERIODIC;
    a.pery = g.bc[CSIM_BOTTOM] == CSIM_BC_PERIODIC && g.bc[CSIM_TOP] == CSIM_BC_PERIODIC;
    int rc = csim_ensemble_perturb_taps(e->dx, corr_len, g.nx, a.perx, &a.rx, a.tx);
    if (!rc) rc = csim_ensemble_perturb_taps(e->dy, corr_len, g.ny, a.pery, &a.ry, a.ty);
    if (rc) return rc;
    if (sigma == 0.0) return CSIM_OK;
    a.seed_lo = static_cast<unsigned>(seed), a.seed_hi = static_cast<unsigned>(seed >> 32), a.draw = draw;
    a.forecast = M;
    a.truth_member = truth_member >= 0 ? truth_member : B;
    a.sigma = sigma;
    CSIM_HIP(ens_launch_perturb(g, e->base(e->cur), a, centered == 1, e->st));
    return CSIM_OK;
}

int csim_ensemble_prior_capture(csim_ensemble* e, int mode, int truth_member) {
    CSIM_REQUIRE(e, "null ensemble");
    const EnsGeom& g = e->g;
    int M = 0;
    int rc = relax_check(e, mode, truth_member, &M);
    if (rc) return rc;
    // each buffer is created once; a failed allocation is reported and retried by the next call
    if (mode == CSIM_RELAX_SPREAD && !e->rx_sb)
        CSIM_HIP(hipMalloc(reinterpret_cast<void**>(&e->rx_sb), sizeof(double) * static_cast<size_t>(g.nx) * g.ny));
    const size_t bytes = sizeof(double) * static_cast<size_t>(g.slab) * g.members;
    if (mode == CSIM_RELAX_PERT && !e->rx_prior) CSIM_HIP(hipMalloc(reinterpret_cast<void**>(&e->rx_prior), bytes));
    e->rx_mode = 0;  // from here on the last capture is being overwritten (in stream order, after its readers)
    if (mode == CSIM_RELAX_SPREAD)
        CSIM_HIP(ens_launch_relax_capture(g, e->base(e->cur), M, truth_member >= 0 ? truth_member : g.members, e->rx_sb,
                                          e->st));
    else
        CSIM_HIP(hipMemcpyAsync(e->rx_prior, e->alloc[e->cur], bytes, hipMemcpyDeviceToDevice, e->st));
    e->rx_mode = mode;
    e->rx_truth = truth_member;
    return CSIM_OK;
}

int csim_ensemble_relax(csim_ensemble* e, int mode, double alpha, int truth_member, double* out_factor) {
    CSIM_REQUIRE(e, "null ensemble");
    const EnsGeom& g = e->g;
    int M = 0;
    int rc = relax_check(e, mode, truth_member, &M);
    if (rc) return rc;
    CSIM_REQUIRE(std::isfinite(alpha) && alpha >= 0.0 && alpha <= 1.0, "alpha must be in [0, 1]");
    CSIM_REQUIRE(!(out_factor && mode == CSIM_RELAX_PERT), "out_factor is for CSIM_RELAX_SPREAD only");
    if (e->rx_mode != mode || e->rx_truth != truth_member)
        return fail(CSIM_ERR_STATE, "csim_ensemble_relax: no valid capture of this mode and truth member "
                                    "(csim_ensemble_prior_capture after the last run)");
    const size_t cells = stats_cells(e);
    if (alpha == 0.0) {
        if (!out_factor) return CSIM_OK;
        std::fill(out_factor, out_factor + cells, 0.0);
        return csim_ensemble_sync(e);
    }
    if (out_factor && !e->rx_factor)
        CSIM_HIP(hipMalloc(reinterpret_cast<void**>(&e->rx_factor), sizeof(double) * cells));
    // Only interior cells of the forecast members in the current buffer are written, as in csim_ensemble_assimilate:
    // ring_ok is only ever true for rings without a Neumann side, whose ghosts do not depend on the interior, Neumann
    // rings are rebuilt from the interior before every pass, and the FinLines were consumed by the ghost fill that ended
    // the run that wrote them, so nothing cached goes stale.
    const int t = truth_member >= 0 ? truth_member : g.members;
    if (mode == CSIM_RELAX_PERT) {
        CSIM_HIP(ens_launch_relax_pert(g, e->base(e->cur), e->rx_prior + static_cast<size_t>(GHOST_EXTRA) * g.pitch, M, t,
                                       alpha, e->st));
        return CSIM_OK;
    }
    if (out_factor) CSIM_HIP(hipMemsetAsync(e->rx_factor, 0, sizeof(double) * cells, e->st));  // the ghost ring: +0
    CSIM_HIP(ens_launch_relax_spread(g, e->base(e->cur), M, t, alpha, e->rx_sb, out_factor ? e->rx_factor : nullptr,
                                     e->st));
    if (!out_factor) return CSIM_OK;
    // as csim_ensemble_stats: copied in stream order, and the call waits for it
    CSIM_HIP(hipMemcpyAsync(out_factor, e->rx_factor, sizeof(double) * cells, hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    return CSIM_OK;
}

int csim_ensemble_set_option(csim_ensemble* e, const char* key, long value) {
    CSIM_REQUIRE(e && key, "null argument");
    const std::string k(key);
    if (k == "fuse") {
        CSIM_REQUIRE(value >= -1 && value <= 1, "fuse must be -1 (auto), 0 or 1");
        e->fuse = static_cast<int>(value);
    } else if (k == "fused_2c") {
        CSIM_REQUIRE(value == 0 || value == 1, "fused_2c must be 0 or 1");
        e->fused_2c = static_cast<int>(value);
        e->dirty = true;
    } else if (k == "depth_used") {
        return fail(CSIM_ERR_ARG, "option depth_used is read-only");
    } else if (k == "contract") {
        return fail(CSIM_ERR_UNSUPPORTED, "an ensemble is always bit-identical: no contract mode");
    } else {
        return fail(CSIM_ERR_ARG, "unknown option " + k);
    }
    return CSIM_OK;
}

int csim_ensemble_get_option(const csim_ensemble* e, const char* key, long* value) {
    CSIM_REQUIRE(e && key && value, "null argument");
    const std::string k(key);
    if (k == "fuse")
        *value = e->fuse;
    else if (k == "fused_2c")
        *value = e->fused_2c;
    else if (k == "depth_used")
        *value = e->depth_used;
    else if (k == "contract")
        return fail(CSIM_ERR_UNSUPPORTED, "an ensemble is always bit-identical: no contract mode");
    else
        return fail(CSIM_ERR_ARG, "unknown option " + k);
    return CSIM_OK;
}

}  // extern "C"
