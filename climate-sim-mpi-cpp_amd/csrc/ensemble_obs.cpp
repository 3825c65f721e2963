// ensemble_obs.cpp — the observation network (csim_obs_network_* of include/csim.h; the type is obs_network.hpp's, the
// kernels are in ensemble_obs.hip): observations that are planned once and live on the device.  create builds the
// plan that csim_ensemble_assimilate builds per call (assim_plan_build of assim_plan.hpp) and uploads it; here are also
// its values (from the host or observed from a member), the mask of csim_obs_network_set_active, and what comes back:
// fetch, the two logs and the status bytes; and the time slots with the rows held at their times (set_slots, hold,
// observe_slot, held; kernels in ensemble_held.hip), which csim_ensemble_assimilate_etkf_held reads.  The analyses that
// run on a network are ensemble_analysis.cpp, the forecast impact is ensemble_obs_impact.cpp.
#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "ensemble_noise.hpp"
#include "obs_network.hpp"

using namespace csim;

namespace {

static_assert(sizeof(csim_obs_cycle) == sizeof(double) * OBS_CYCLE_FIELDS, "csim_obs_cycle is 13 doubles");
static_assert(sizeof(csim_obs_screen_cycle) == sizeof(double) * OBS_SCREEN_FIELDS, "csim_obs_screen_cycle is 3 doubles");

// the decision of csim_ensemble_assimilate_screened for one observation, as k_obs_screen makes it
int screen_decide(double y, double hb, double vb, double r, double tol, bool active) {
    if (!active) return CSIM_OBS_INACTIVE;
    if (!(tol > 0)) return CSIM_OBS_USED;
    const double k2 = tol * tol;
    const double t = y - hb;
    const double lhs = t * t;
    const double rhs = k2 * (vb + r);
    return lhs <= rhs ? CSIM_OBS_USED : CSIM_OBS_REJECTED;
}

}  // namespace

void csim_ensemble::Obs::release() {
    for (csim_obs_network* n : nets) delete n;
    nets.clear();
}

namespace {

// nobs values in plan order on the device -> input order on the host; the stream is idle afterwards
template <class T> int fetch_plan_order(const csim_obs_network* n, size_t byte, T* out) {
    std::vector<T> buf(n->nobs);
    CSIM_HIP(hipMemcpyAsync(buf.data(), n->at<char>(byte), sizeof(T) * buf.size(), hipMemcpyDeviceToHost, n->e->st));
    CSIM_HIP(hipStreamSynchronize(n->e->st));
    for (int q = 0; q < n->nobs; ++q) out[n->idx[q]] = buf[q];
    return CSIM_OK;
}

// (mean, variance) pairs by input index on the device -> two host arrays, either may be null
int fetch_pairs(const csim_obs_network* n, size_t byte, double* mean, double* var) {
    if (!mean && !var) return CSIM_OK;
    std::vector<double> buf(2 * static_cast<size_t>(n->nobs));
    CSIM_HIP(hipMemcpyAsync(buf.data(), n->at<char>(byte), sizeof(double) * buf.size(), hipMemcpyDeviceToHost, n->e->st));
    CSIM_HIP(hipStreamSynchronize(n->e->st));
    split_pairs(buf.data(), n->nobs, mean, var);
    return CSIM_OK;
}

// csim_obs_network_log and _screen_log: the first min(max, cycles) records, `record` bytes each, of the log at l.*log
int fetch_log(csim_obs_network* n, size_t ObsLayout::*log, size_t record, int max, void* out, int* ncycles) {
    CSIM_REQUIRE(n, "null network");
    CSIM_REQUIRE(max >= 0 && (max == 0 || out), "max must be >= 0, with room for that many records");
    CSIM_HIP(hipStreamSynchronize(n->e->st));
    const int k = std::min(max, n->cycles);
    if (k > 0) {
        CSIM_HIP(hipMemcpyAsync(out, n->at<char>(n->l.*log), record * k, hipMemcpyDeviceToHost, n->e->st));
        CSIM_HIP(hipStreamSynchronize(n->e->st));
    }
    if (ncycles) *ncycles = n->cycles;
    return CSIM_OK;
}

// the taps of csim_obs_network_create_linear, input order
struct Taps {
    const int *start, *di, *dj;
    const double* w;
};

// csim_obs_network_create (taps null) and csim_obs_network_create_linear
int network_create(csim_ensemble* e, int nobs, const int* i, const int* j, const Taps* taps, const double* r, double loc,
                   int ordered, int log_cycles, csim_obs_network** out) {
    CSIM_REQUIRE(out, "out is null");
    *out = nullptr;
    CSIM_REQUIRE(e, "null ensemble");
    const EnsGeom& g = e->g;
    CSIM_REQUIRE(nobs >= 1, "nobs must be >= 1");
    CSIM_REQUIRE(i && j && r, "null observation array");
    CSIM_REQUIRE(!taps || (taps->start && taps->di && taps->dj && taps->w), "null tap array");
    CSIM_REQUIRE(!taps || g.slab <= 0x7fffffffL, "grid too large for packed tap offsets");
    CSIM_REQUIRE(std::isfinite(loc) && loc > 0, "loc must be finite and > 0");
    CSIM_REQUIRE(ordered == 0 || ordered == 1, "ordered must be 0 or 1");
    CSIM_REQUIRE(log_cycles >= 0 && log_cycles <= 65536, "log_cycles must be in 0 .. 65536");
    if (nobs > ASSIM_MAX_OBS) return fail(CSIM_ERR_UNSUPPORTED, "csim_obs_network_create: at most 2^20 observations");
    // the network is the caller's only once everything has worked; no exception crosses the C ABI
    try {
        std::unique_ptr<csim_obs_network> n(new csim_obs_network);
        CSIM_TRY(assim_plan_build(g.nx, g.ny, e->dx, e->dy, loc, ordered == 1, nobs, i, j, r, nullptr, n.get()));
        // the taps need the half-widths; nothing that the builder does after its checks of the observations can fail,
        // so their check fires where it did, after those
        if (taps)
            CSIM_TRY(csim_obs_linear_check(g.nx, g.ny, n->lx, n->ly, nobs, i, j, taps->start, taps->di, taps->dj, taps->w));
        n->e = e, n->log_cycles = log_cycles;
        // h'_k of the largest batch of either number of forecast members
        size_t hp = 0;
        for (int M = g.members - 1; M <= g.members; ++M)
            if (M >= 2 && M <= ASSIM_MAX_MEMBERS)
                hp = std::max(hp, static_cast<size_t>(std::min(nobs, assim_batch_size(M))) * M);
        const size_t tcells = static_cast<size_t>(2 * n->lx + 1) * (2 * n->ly + 1);
        if (taps) {
            n->ntaps = taps->start[nobs];
            for (int o = 0; o < nobs; ++o) n->tmax = std::max(n->tmax, taps->start[o + 1] - taps->start[o]);
        }
        const size_t chunks = (static_cast<size_t>(nobs) + OBS_CHUNK - 1) / OBS_CHUNK;
        n->l = obs_layout(nobs, n->ntaps, tcells, hp, OBS_SUMS * chunks,
                          static_cast<size_t>(OBS_CYCLE_FIELDS) * log_cycles, OBS_SCREEN_FIELDS * chunks,
                          static_cast<size_t>(OBS_SCREEN_FIELDS) * log_cycles);
        const ObsLayout& l = n->l;
        std::vector<char> h(l.fixed, 0);
        std::copy(n->pi.begin(), n->pi.end(), buf_at<int>(h.data(), l.i));
        std::copy(n->pj.begin(), n->pj.end(), buf_at<int>(h.data(), l.j));
        std::copy(n->idx.begin(), n->idx.end(), buf_at<int>(h.data(), l.idx));
        int* hpos = buf_at<int>(h.data(), l.pos);
        double *hr = buf_at<double>(h.data(), l.r), *hs = buf_at<double>(h.data(), l.sr);
        for (int q = 0; q < nobs; ++q) {
            const int o = n->idx[q];
            hpos[o] = q, hr[q] = r[o], hs[q] = std::sqrt(r[o]);
        }
        if (taps)
            obs_taps_plan_order(nobs, n->idx.data(), taps->start, taps->di, taps->dj, taps->w, g.pitch,
                                buf_at<int>(h.data(), l.tstart), buf_at<int>(h.data(), l.toff),
                                buf_at<double>(h.data(), l.tw));
        gc_fill(e->dx, e->dy, loc, n->lx, n->ly, buf_at<double>(h.data(), l.rho));
        CSIM_TRY(n->dev.reserve(l.total));
        hipError_t err = hipMemsetAsync(n->dev.p, 0, l.total, e->st);
        if (err == hipSuccess) err = hipMemcpyAsync(n->dev.p, h.data(), l.fixed, hipMemcpyHostToDevice, e->st);
        if (err == hipSuccess) err = ens_launch_obs_screen_log_fill(n->at<double>(l.slog), log_cycles, nobs, e->st);
        if (err == hipSuccess) err = hipStreamSynchronize(e->st);  // h goes away
        if (err != hipSuccess) return fail(CSIM_ERR_HIP, std::string("csim_obs_network_create: ") + hipGetErrorString(err));
        e->obs.nets.push_back(n.get());
        *out = n.release();
        return CSIM_OK;
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, "csim_obs_network_create: out of host memory");
    }
}

// the observations of `slot` (-1: all) as a launch: their number and the device list of their plan positions (null: the
// positions 0 .. count - 1 themselves)
void slot_launch(const csim_obs_network* n, int slot, int* count, const int** list) {
    const csim_obs_network::Held& x = n->hold;
    *list = nullptr;
    if (slot < 0 || (x.start.empty() && slot == 0)) {
        *count = n->nobs;
    } else if (x.start.empty()) {
        *count = 0;
    } else {
        *count = x.start[slot + 1] - x.start[slot];
        *list = x.list.cpos() + x.start[slot];
    }
}

}  // namespace

extern "C" {

int csim_obs_network_create(csim_ensemble* e, int nobs, const int* i, const int* j, const double* r, double loc,
                            int ordered, int log_cycles, csim_obs_network** out) {
    return network_create(e, nobs, i, j, nullptr, r, loc, ordered, log_cycles, out);
}

int csim_obs_network_create_linear(csim_ensemble* e, int nobs, const int* i, const int* j, const int* start,
                                   const int* di, const int* dj, const double* w, const double* r, double loc,
                                   int ordered, int log_cycles, csim_obs_network** out) {
    const Taps taps{start, di, dj, w};
    return network_create(e, nobs, i, j, &taps, r, loc, ordered, log_cycles, out);
}

int csim_obs_network_taps(const csim_obs_network* n, int* ntaps_total) {
    CSIM_REQUIRE(n, "null network");
    CSIM_REQUIRE(ntaps_total, "null argument");
    *ntaps_total = n->ntaps;
    return CSIM_OK;
}

int csim_obs_network_destroy(csim_obs_network* n) {
    if (!n) return CSIM_OK;
    csim_ensemble* e = n->e;
    if (e->st) (void)hipStreamSynchronize(e->st);  // work enqueued there may still use the buffer
    e->obs.nets.erase(std::remove(e->obs.nets.begin(), e->obs.nets.end(), n), e->obs.nets.end());
    delete n;
    return CSIM_OK;
}

int csim_obs_network_info(const csim_obs_network* n, int* nobs, int* nlevels, int* lx, int* ly) {
    CSIM_REQUIRE(n, "null network");
    if (nobs) *nobs = n->nobs;
    if (nlevels) *nlevels = n->nlevels;
    if (lx) *lx = n->lx;
    if (ly) *ly = n->ly;
    return CSIM_OK;
}

int csim_obs_network_set_values(csim_obs_network* n, const double* y) {
    CSIM_REQUIRE(n, "null network");
    CSIM_REQUIRE(y, "null values");
    for (int o = 0; o < n->nobs; ++o) CSIM_REQUIRE(std::isfinite(y[o]), "observation value must be finite");
    void* staged = nullptr;
    CSIM_TRY(n->stage.acquire(sizeof(double) * n->nobs, &staged));
    auto* hy = static_cast<double*>(staged);
    for (int q = 0; q < n->nobs; ++q) hy[q] = y[n->idx[q]];
    CSIM_TRY(n->stage.send(n->at<char>(n->l.y), sizeof(double) * n->nobs, n->e->st));
    n->has_values = true;
    n->has_truth = false;
    n->hold.seen = 0;
    return CSIM_OK;
}

int csim_obs_network_set_active(csim_obs_network* n, const unsigned char* active) {
    CSIM_REQUIRE(n, "null network");
    bool any = false;
    if (active)
        for (int o = 0; o < n->nobs; ++o) {
            CSIM_REQUIRE(active[o] <= 1, "a mask byte must be 0 or 1");
            any = any || !active[o];
        }
    if (!any) {  // all active: the mask on the device is not read
        n->masked = false;
        return CSIM_OK;
    }
    void* staged = nullptr;
    CSIM_TRY(n->mstage.acquire(n->nobs, &staged));
    auto* hm = static_cast<unsigned char*>(staged);
    for (int q = 0; q < n->nobs; ++q) hm[q] = active[n->idx[q]];
    CSIM_TRY(n->mstage.send(n->at<char>(n->l.mask), n->nobs, n->e->st));
    n->masked = true;
    return CSIM_OK;
}

int csim_obs_network_observe(csim_obs_network* n, int source_member, unsigned long long seed, unsigned draw,
                             int noise) {
    CSIM_REQUIRE(n, "null network");
    csim_ensemble* e = n->e;
    CSIM_REQUIRE(source_member >= 0 && source_member < e->g.members, "source_member out of range");
    CSIM_REQUIRE(noise == 0 || noise == 1, "noise must be 0 or 1");
    CSIM_HIP(ens_launch_obs_observe(e->g, e->base(e->cur), n->args(), source_member, static_cast<unsigned>(seed),
                                    static_cast<unsigned>(seed >> 32), draw, noise == 1, e->st));
    n->has_values = true;
    n->has_truth = true;
    return CSIM_OK;
}

int csim_obs_slots_present(int nobs, const int* slot, unsigned long long* mask) {
    CSIM_REQUIRE(nobs >= 1, "nobs must be >= 1");
    CSIM_REQUIRE(mask, "null argument");
    unsigned long long m = slot ? 0ull : 1ull;
    if (slot)
        for (int o = 0; o < nobs; ++o) {
            CSIM_REQUIRE(slot[o] >= 0 && slot[o] < CSIM_OBS_MAX_SLOTS, "a slot must be in 0 .. CSIM_OBS_MAX_SLOTS - 1");
            m |= 1ull << slot[o];
        }
    *mask = m;
    return CSIM_OK;
}

int csim_obs_network_set_slots(csim_obs_network* n, const int* slot) {
    CSIM_REQUIRE(n, "null network");
    unsigned long long present = 1;
    CSIM_TRY(csim_obs_slots_present(n->nobs, slot, &present));
    csim_obs_network::Held& x = n->hold;
    try {
        // the plan positions grouped by slot, increasing within one; all in slot 0: no list, a position is its own entry
        std::vector<int> start, pos;
        if (slot && present != 1ull) {
            start.assign(CSIM_OBS_MAX_SLOTS + 1, 0);
            pos.resize(n->nobs);
            for (int o = 0; o < n->nobs; ++o) ++start[slot[o] + 1];
            for (int s = 0; s < CSIM_OBS_MAX_SLOTS; ++s) start[s + 1] += start[s];
            std::vector<int> at(start.begin(), start.end() - 1);
            for (int q = 0; q < n->nobs; ++q) pos[at[slot[n->idx[q]]]++] = q;
            CSIM_TRY(x.list.upload(start, pos, 1, n->e->st));
        } else {
            x.list.key = 0;
        }
        x.start.swap(start);
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, "csim_obs_network_set_slots: out of host memory");
    }
    x.present = present, x.held = 0, x.seen = 0, x.done = false;
    return CSIM_OK;
}

int csim_obs_network_hold(csim_obs_network* n, int slot, int truth_member) {
    CSIM_REQUIRE(n, "null network");
    CSIM_REQUIRE(slot >= -1 && slot < CSIM_OBS_MAX_SLOTS, "slot must be -1 or in 0 .. CSIM_OBS_MAX_SLOTS - 1");
    csim_ensemble* e = n->e;
    int M = 0, t = 0;
    CSIM_TRY(forecast_split(e->g.members, truth_member, &M, &t));
    if (M < 2 || M > ESPACE_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_obs_network_hold: 2 .. CSIM_ESPACE_MAX_MEMBERS forecast members");
    const size_t doubles = static_cast<size_t>(n->nobs) * M;
    if (doubles > static_cast<size_t>(CSIM_LOCAL_MAX_PRIOR_DOUBLES))
        return fail(CSIM_ERR_UNSUPPORTED, "csim_obs_network_hold: nobs times the forecast members exceeds "
                                          "CSIM_LOCAL_MAX_PRIOR_DOUBLES");
    csim_obs_network::Held& x = n->hold;
    if (x.M != M || x.t != t) x.held = 0;  // rows of other members are forgotten
    if (sizeof(double) * doubles > x.rows.cap) x.held = 0, x.M = 0;  // a buffer that grows loses its rows
    CSIM_TRY(x.rows.reserve(sizeof(double) * doubles, e->st));
    x.M = M, x.t = t;
    int count = 0;
    const int* list = nullptr;
    slot_launch(n, slot, &count, &list);
    const ObsArgs oa = n->args();
    const AssimArgs a = assim_args(M, t, *n, n->at<double>(n->l.rho), {oa.i, oa.j, oa.idx, oa.y, oa.r}, nullptr, nullptr,
                                   nullptr, oa.tstart, oa.toff, oa.tw, n->tmax);
    CSIM_HIP(ens_launch_obs_hold(e->g, e->base(e->cur), a, list, count, x.rows.as(), e->st));
    x.held |= slot < 0 ? ~0ull : 1ull << slot;
    x.done = false;
    return CSIM_OK;
}

int csim_obs_network_observe_slot(csim_obs_network* n, int slot, int source_member, unsigned long long seed,
                                  unsigned draw, int noise) {
    CSIM_REQUIRE(n, "null network");
    CSIM_REQUIRE(slot >= 0 && slot < CSIM_OBS_MAX_SLOTS, "slot must be in 0 .. CSIM_OBS_MAX_SLOTS - 1");
    csim_ensemble* e = n->e;
    CSIM_REQUIRE(source_member >= 0 && source_member < e->g.members, "source_member out of range");
    CSIM_REQUIRE(noise == 0 || noise == 1, "noise must be 0 or 1");
    int count = 0;
    const int* list = nullptr;
    slot_launch(n, slot, &count, &list);
    if (!list && count)
        CSIM_HIP(ens_launch_obs_observe(e->g, e->base(e->cur), n->args(), source_member, static_cast<unsigned>(seed),
                                        static_cast<unsigned>(seed >> 32), draw, noise == 1, e->st));
    else
        CSIM_HIP(ens_launch_obs_observe_list(e->g, e->base(e->cur), n->args(), list, count, source_member,
                                             static_cast<unsigned>(seed), static_cast<unsigned>(seed >> 32), draw,
                                             noise == 1, e->st));
    csim_obs_network::Held& x = n->hold;
    x.seen |= 1ull << slot;
    if ((x.seen & x.present) == x.present) n->has_values = true, n->has_truth = true;
    return CSIM_OK;
}

int csim_obs_network_held(csim_obs_network* n, double* H, int* M, int* truth_member) {
    CSIM_REQUIRE(n, "null network");
    const csim_obs_network::Held& x = n->hold;
    // after a held analysis no slot counts as held, but its transformed rows stay until the next hold
    if (!x.M || !(x.all_held() || x.done))
        return fail(CSIM_ERR_STATE, "csim_obs_network_held: not every slot that occurs has been held "
                                    "(csim_obs_network_hold)");
    if (M) *M = x.M;
    if (truth_member) *truth_member = x.t < n->e->g.members ? x.t : -1;
    CSIM_HIP(hipStreamSynchronize(n->e->st));
    if (!H) return CSIM_OK;
    try {
        const size_t m = static_cast<size_t>(x.M);
        std::vector<double> buf(m * n->nobs);
        CSIM_HIP(hipMemcpyAsync(buf.data(), x.rows.p, sizeof(double) * buf.size(), hipMemcpyDeviceToHost, n->e->st));
        CSIM_HIP(hipStreamSynchronize(n->e->st));
        for (int q = 0; q < n->nobs; ++q) std::copy(buf.begin() + q * m, buf.begin() + (q + 1) * m, H + n->idx[q] * m);
        return CSIM_OK;
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, "csim_obs_network_held: out of host memory");
    }
}

int csim_obs_noise(unsigned long long seed, unsigned draw, unsigned o, double* z) {
    CSIM_REQUIRE(z, "null argument");
    unsigned c[4] = {o, 0u, 0xFFFFFFFFu, draw};
    philox4x32(c, static_cast<unsigned>(seed), static_cast<unsigned>(seed >> 32));
    *z = normal_from_bits(static_cast<unsigned long long>(c[0]) | (static_cast<unsigned long long>(c[1]) << 32));
    return CSIM_OK;
}

int csim_obs_screen_decide(double y, double hb, double vb, double r, double tol, int active, int* status) {
    CSIM_REQUIRE(status, "null argument");
    CSIM_REQUIRE(std::isfinite(tol) && tol >= 0, "tol must be finite and >= 0");
    CSIM_REQUIRE(active == 0 || active == 1, "active must be 0 or 1");
    *status = screen_decide(y, hb, vb, r, tol, active == 1);
    return CSIM_OK;
}

int csim_obs_network_fetch(csim_obs_network* n, double* y, double* truth, double* bg_mean, double* bg_var,
                           double* post_mean, double* post_var) {
    CSIM_REQUIRE(n, "null network");
    if (y && !n->has_values) return fail(CSIM_ERR_STATE, "csim_obs_network_fetch: the network has no values yet");
    if (truth && !n->has_truth)
        return fail(CSIM_ERR_STATE, "csim_obs_network_fetch: the values were not observed from a member");
    if ((bg_mean || bg_var || post_mean || post_var) && !n->has_diag)
        return fail(CSIM_ERR_STATE, "csim_obs_network_fetch: no analysis has been recorded");
    CSIM_HIP(hipStreamSynchronize(n->e->st));
    if (y) CSIM_TRY(fetch_plan_order(n, n->l.y, y));
    if (truth) CSIM_TRY(fetch_plan_order(n, n->l.xt, truth));
    CSIM_TRY(fetch_pairs(n, n->l.bg, bg_mean, bg_var));
    CSIM_TRY(fetch_pairs(n, n->l.post, post_mean, post_var));
    return CSIM_OK;
}

int csim_obs_network_log(csim_obs_network* n, int max, csim_obs_cycle* out, int* ncycles) {
    return fetch_log(n, &ObsLayout::log, sizeof(csim_obs_cycle), max, out, ncycles);
}

int csim_obs_network_log_reset(csim_obs_network* n) {
    CSIM_REQUIRE(n, "null network");
    if (n->log_cycles) {
        CSIM_HIP(hipMemsetAsync(n->at<char>(n->l.log), 0, sizeof(csim_obs_cycle) * n->log_cycles, n->e->st));
        CSIM_HIP(ens_launch_obs_screen_log_fill(n->at<double>(n->l.slog), n->log_cycles, n->nobs, n->e->st));
    }
    n->cycles = 0;
    return CSIM_OK;
}

int csim_obs_network_screen_log(csim_obs_network* n, int max, csim_obs_screen_cycle* out, int* ncycles) {
    return fetch_log(n, &ObsLayout::slog, sizeof(csim_obs_screen_cycle), max, out, ncycles);
}

int csim_obs_network_status(csim_obs_network* n, unsigned char* status) {
    CSIM_REQUIRE(n, "null network");
    CSIM_REQUIRE(status, "null argument");
    if (!n->analysed) return fail(CSIM_ERR_STATE, "csim_obs_network_status: the network has not been analysed yet");
    CSIM_HIP(hipStreamSynchronize(n->e->st));
    if (!n->screened) {  // nothing was screened: every observation was used
        std::fill(status, status + n->nobs, static_cast<unsigned char>(CSIM_OBS_USED));
        return CSIM_OK;
    }
    return fetch_plan_order(n, n->l.status, status);
}

}  // extern "C"
