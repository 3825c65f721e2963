// ensemble_obs.cpp — the observation network (csim_obs_network_* and csim_ensemble_assimilate_network of include/csim.h;
// kernels in ensemble_obs.hip): observations that are planned once and live on the device.  create builds the
// plan that csim_ensemble_assimilate builds per call (assim_plan_build of assim_plan.hpp) and uploads it; the analysis
// then only points an AssimArgs into the network's buffer and enqueues the launches of ensemble_da.cpp's assim_enqueue.
// Screening (csim_obs_network_set_active, csim_ensemble_assimilate_screened) adds a mask and a status byte per plan
// position: one k_obs_screen launch ahead of the analysis, whose kernels then skip what is not used.
// The forecast impact (csim_obs_network_impact_capture, csim_ensemble_obs_impact; kernels in ensemble_impact.hip) keeps
// a capture in storage of the network's own, made at the first capture: a_k per observation, dn and the status bytes,
// and a device copy of the caller's weight; nothing that an analysis, observe or set_values writes.
// csim_ensemble_obs_impact_global reads the same capture without the localisation: the weight goes through the
// ensemble-space dot (dot_stage_fields, dot_enqueue of ensemble_space.cpp), then one kernel of ensemble_dot.hip.  The
// two calls differ in that, the staging of the weight and the launch; their checks and what they bring back are one
// text (impact_check, impact_run).
// Four more analyses share the checks, the screening and the recording of the serial one (analysis_check,
// analysis_begin, analysis_record) and differ in what runs between them:
//   local  (ensemble_local.hip)  the observation priors and a lookup per tile, storage of the network's own
//   ETKF   the observation-space Gram matrix of the used observations (csim_ensemble_obs_gram, ensemble_obsgram.hip,
//          which writes nothing of the network), csim_etkf_weights on the host, csim_ensemble_transform; or, _device,
//          the eigensolver and the weights of sym_eigen_device.hip with no host round trip
//   LETKF  (ensemble_letkf.hip)  the local analysis's priors, a Gram matrix per node of a lattice, the batched
//          eigensolver and weights, and a cell pass that interpolates the weights; a lookup per spacing
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "ensemble_host.hpp"
#include "ensemble_noise.hpp"
#include "sym_eigen.hpp"

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

// the lane-and-butterfly sum of csim_ensemble_obs_impact: what one wave of k_obs_impact does with its cells
double impact_fold(const double* u, long n) {
    double l[64];
    for (int j = 0; j < 64; ++j) l[j] = 0.0;
    for (long e = 0; e < n; ++e) l[e % 64] = l[e % 64] + u[e];
    for (int h = 32; h >= 1; h >>= 1) {
        double m[64];
        for (int j = 0; j < 64; ++j) m[j] = l[j] + l[j ^ h];
        for (int j = 0; j < 64; ++j) l[j] = m[j];
    }
    return l[0];
}

// a lookup on the device (LocalTiles, LetkfLookup): its starts, then its plan positions
struct DeviceLookup {
    DeviceBuf buf;
    Staging stage;
    size_t pos_at = 0;  // where the plan positions start, bytes
    int key = 0;        // what it was built for (a tile, a spacing; 0: none)
    void release() { buf.release(), stage.release(); }
    const int* cstart() const { return buf_at<int>(buf.p, 0); }
    const int* cpos() const { return buf_at<int>(buf.p, pos_at); }
    int upload(const std::vector<int>& start, const std::vector<int>& pos, int k, hipStream_t st) {
        const size_t at = up(sizeof(int) * start.size()), bytes = up(at + sizeof(int) * pos.size());
        void* staged = nullptr;
        CSIM_TRY(stage.acquire(bytes, &staged));
        std::copy(start.begin(), start.end(), buf_at<int>(staged, 0));
        std::copy(pos.begin(), pos.end(), buf_at<int>(staged, at));
        key = 0;  // from here on the last lookup is being replaced (after its readers)
        CSIM_TRY(buf.reserve(bytes, st));
        CSIM_TRY(stage.send(buf.p, bytes, st));
        key = k, pos_at = at;
        return CSIM_OK;
    }
};

}  // namespace

struct csim_obs_network : AssimPlan {   // the plan: nobs, nlevels, lx, ly, off, idx, pi, pj
    csim_ensemble* e = nullptr;
    int log_cycles = 0, ntaps = 0, tmax = 0;  // ntaps, tmax: a linear network's taps in all, the most of one observation
    std::vector<AssimBatch> batches;    // its launches for batches_m forecast members (made at the first analysis)
    int batches_m = 0;
    ObsLayout l{};
    DeviceBuf dev;
    Staging stage;                      // of set_values
    Staging mstage;                     // of set_active
    bool has_values = false, has_truth = false, has_diag = false;
    bool masked = false;                // the mask on the device has an inactive observation (else it is not read)
    bool analysed = false, screened = false;  // there was an analysis; the last one launched the screening
    int cycles = 0;                     // records in both logs
    bool last_recorded = false;         // the last analysis was a recorded one: bg and the status bytes are its own
    // the capture of csim_obs_network_impact_capture, made at the first capture and kept until destroy
    struct Impact {
        DeviceBuf pert;                 // M doubles per plan position: a_k
        DeviceBuf aux;                  // dn (plan order), J (input order), the status snapshot (plan order)
        DeviceBuf w;                    // the weight of the last csim_ensemble_obs_impact, dense
        Staging wstage;
        bool valid = false;
        int M = 0, t = 0;               // its forecast members: M of them, member t left out (t = B: none)
        void release() { pert.release(), aux.release(), w.release(), wstage.release(); }
    } imp;
    // the local analysis (csim_ensemble_assimilate_local), made at the first one and kept until destroy
    struct Local {
        int max_local = -1;             // the most window rectangles over one cell (-1: not counted yet)
        DeviceBuf prior;                // M doubles per plan position: h_{o,k}
        DeviceLookup tiles;             // the lookup (LocalTiles), its key the tile
        int ntx = 0, nty = 0;           // of the lookup on the device
        void release() { prior.release(), tiles.release(); }
    } loc;
    // the LETKF (csim_ensemble_assimilate_letkf): the lookup of the last spacing, made when the spacing is another one
    // and kept until destroy; the observation priors are those of the local analysis (loc.prior)
    struct Letkf {
        DeviceLookup nodes;             // the lookup (LetkfLookup), its key the spacing
        void release() { nodes.release(); }
    } letkf;
    size_t imp_dn() const { return 0; }
    size_t imp_out() const { return up(sizeof(double) * nobs); }
    size_t imp_snap() const { return 2 * up(sizeof(double) * nobs); }
    size_t imp_bytes() const { return imp_snap() + up(nobs); }
    template <class T> T* at(size_t byte) const { return buf_at<T>(dev.p, byte); }
    ObsArgs args() const {
        ObsArgs a{};
        a.nobs = nobs;
        a.i = at<int>(l.i), a.j = at<int>(l.j), a.idx = at<int>(l.idx), a.pos = at<int>(l.pos);
        a.r = at<double>(l.r), a.sr = at<double>(l.sr);
        a.y = at<double>(l.y), a.xt = at<double>(l.xt);
        a.bg = at<double>(l.bg), a.post = at<double>(l.post), a.part = at<double>(l.part);
        if (ntaps) a.tstart = at<int>(l.tstart), a.toff = at<int>(l.toff), a.tw = at<double>(l.tw);
        return a;
    }
    ~csim_obs_network() { dev.release(), stage.release(), mstage.release(), imp.release(), loc.release(), letkf.release(); }
};

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

// What csim_ensemble_assimilate_screened and csim_ensemble_assimilate_local share.  The argument and state checks, in
// the order they fire; M forecast members without member t
int analysis_check(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member, int record, double tol,
                   int* M, int* t) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_REQUIRE(n, "null network");
    CSIM_REQUIRE(n->e == e, "the network belongs to another ensemble");
    CSIM_REQUIRE(std::isfinite(inflation) && inflation >= 1.0, "inflation must be finite and >= 1");
    CSIM_TRY(forecast_split(e->g.members, truth_member, M, t, 2, "the analysis needs at least two forecast members",
                            ASSIM_MAX_MEMBERS, "csim_ensemble_assimilate_network: at most 1024 forecast members"));
    CSIM_REQUIRE(record == 0 || record == 1, "record must be 0 or 1");
    CSIM_REQUIRE(std::isfinite(tol) && tol >= 0, "tol must be finite and >= 0");
    if (!n->has_values)
        return fail(CSIM_ERR_STATE, "csim_ensemble_assimilate_network: the network has no values yet "
                                    "(csim_obs_network_set_values or csim_obs_network_observe)");
    if (record && n->cycles >= n->log_cycles)
        return fail(CSIM_ERR_STATE, n->log_cycles ? "csim_ensemble_assimilate_network: the log is full"
                                                  : "csim_ensemble_assimilate_network: the network has no log");
    return CSIM_OK;
}

// analysis_check and the member limit of csim_ensemble_assimilate_etkf and _etkf_device
int etkf_check(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member, int record, double tol, int* M,
               int* t) {
    CSIM_TRY(analysis_check(e, n, inflation, truth_member, record, tol, M, t));
    if (*M > ESPACE_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_etkf: at most CSIM_ESPACE_MAX_MEMBERS forecast "
                                          "members");
    return CSIM_OK;
}

// where A is not finite: the host path says so from the analysis, the device path from csim_ensemble_etkf_info
constexpr const char* ETKF_NONFINITE_TEXT = "csim_ensemble_assimilate_etkf: the observation-space Gram matrix has a "
                                            "non-finite entry; the members are unchanged";

// an analysis between its screening and its record
struct Analysis {
    ObsArgs oa;
    AssimArgs a;       // `status` set where the analysis is screened
    ObsScreen s;
    bool screen;
    const double* f;   // the current buffer
};

// the first launches of an analysis: (hb, vb) where they are wanted and the status bytes where something is screened;
// sets the network's flags
int analysis_begin(csim_ensemble* e, csim_obs_network* n, int M, int t, int record, double tol, Analysis* x) {
    x->oa = n->args();
    const ObsArgs& oa = x->oa;
    x->a = assim_args(M, t, *n, n->at<double>(n->l.rho), {oa.i, oa.j, oa.idx, oa.y, oa.r}, n->at<double>(n->l.scal),
                      n->at<double>(n->l.hp), nullptr, oa.tstart, oa.toff, oa.tw, n->tmax);
    x->f = e->base(e->cur);
    // (hb, vb): of a recorded analysis where fetch reads them, of an unrecorded background check where it does not
    const bool check = tol > 0;
    x->screen = check || n->masked;
    double* bg = n->at<double>(record ? n->l.bg : n->l.sbg);
    if (record || check) CSIM_HIP(ens_launch_assim_post(e->g, x->f, x->a, n->nobs, bg, e->st));
    x->s = ObsScreen{};
    if (x->screen) {
        ObsScreen& s = x->s;
        s.mask = n->masked ? n->at<unsigned char>(n->l.mask) : nullptr;
        s.status = n->at<unsigned char>(n->l.status);
        s.bg = bg, s.check = check ? 1 : 0, s.k2 = tol * tol;
        s.cnt = n->at<int>(n->l.cnt);
        CSIM_HIP(ens_launch_obs_screen(oa, s, e->st));
        x->a.status = s.status;
    }
    n->analysed = true, n->screened = x->screen, n->last_recorded = record == 1;
    return CSIM_OK;
}

// the last launches of a recorded analysis: (ha, va) and the cycle's records
int analysis_record(csim_ensemble* e, csim_obs_network* n, const Analysis& x) {
    CSIM_HIP(ens_launch_assim_post(e->g, x.f, x.a, n->nobs, n->at<double>(n->l.post), e->st));
    double* slot = n->at<double>(n->l.log) + static_cast<size_t>(OBS_CYCLE_FIELDS) * n->cycles;
    // the screen record of a cycle that is not screened is the (nobs, 0, 0) that create and log_reset put there
    if (x.screen)
        CSIM_HIP(ens_launch_obs_cycle_screened(x.oa, x.s, n->has_truth, slot, n->at<double>(n->l.slog) +
                                               static_cast<size_t>(OBS_SCREEN_FIELDS) * n->cycles, e->st));
    else
        CSIM_HIP(ens_launch_obs_cycle(x.oa, n->has_truth, slot, e->st));
    ++n->cycles;
    n->has_diag = true;
    return CSIM_OK;
}

// csim_ensemble_obs_gram and step 3 of csim_ensemble_assimilate_etkf: A, loglik (with want_ll) and the count of the
// observations whose flag byte is `used` (flag null: all), synchronous.  *out: (M + 1)^2 + M doubles, A first.  The
// class partials and the result use the buffers of csim_ensemble_gram, which is synchronous as well.
// obs_gram_enqueue only launches and leaves the result in Espace::gram
int obs_gram_enqueue(csim_ensemble* e, csim_obs_network* n, int M, int t, const unsigned char* flag, int used,
                     bool want_ll) {
    csim_ensemble::Espace& x = e->espace;
    const ObsArgs oa = n->args();
    ObsGramArgs a{};
    a.nobs = n->nobs, a.forecast = M, a.truth_member = t;
    a.i = oa.i, a.j = oa.j, a.y = oa.y, a.sr = oa.sr;
    a.flag = flag, a.used = used;
    a.tstart = oa.tstart, a.toff = oa.toff, a.tw = oa.tw;
    const size_t ma = static_cast<size_t>(M) + 1, doubles = ma * ma + M + 1;
    CSIM_TRY(x.partial.reserve(sizeof(double) * ens_obs_gram_partial_doubles(M, n->nobs), e->st));
    CSIM_TRY(x.gram.reserve(sizeof(double) * doubles, e->st));
    CSIM_HIP(ens_launch_obs_gram(e->g, e->base(e->cur), a, want_ll, x.partial.as(), x.gram.as(), x.obs_gram_form, e->st));
    return CSIM_OK;
}

int obs_gram(csim_ensemble* e, csim_obs_network* n, int M, int t, const unsigned char* flag, int used, bool want_ll,
             std::vector<double>* out, long long* n_used) {
    csim_ensemble::Espace& x = e->espace;
    const size_t ma = static_cast<size_t>(M) + 1, doubles = ma * ma + M + 1;
    CSIM_TRY(obs_gram_enqueue(e, n, M, t, flag, used, want_ll));
    out->resize(doubles);
    CSIM_HIP(hipMemcpyAsync(out->data(), x.gram.p, sizeof(double) * doubles, hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    static_assert(sizeof(long long) == sizeof(double), "the count travels behind loglik");
    std::memcpy(n_used, out->data() + ma * ma + M, sizeof(long long));
    return CSIM_OK;
}

// max_local of the network, counted once
int local_max(csim_obs_network* n, int* max_local) {
    if (n->loc.max_local < 0)
        CSIM_TRY(csim_obs_local_count(n->e->g.nx, n->e->g.ny, n->nobs, n->pi.data(), n->pj.data(), n->lx, n->ly, nullptr,
                                      &n->loc.max_local));
    *max_local = n->loc.max_local;
    return CSIM_OK;
}

// the tile of the lookup: the option, or 8 (64 cells fill the last wave of a tile better than 16 do, and a tile's
// entries stay few), 4 on grids too small to give every SIMD a wave that way, 16 on very large ones
int local_tile(const csim_ensemble* e) {
    if (e->local.tile) return e->local.tile;
    const long cells = static_cast<long>(e->g.nx) * e->g.ny;
    return cells >= 2048L * 2048 ? 16 : cells >= 128L * 128 ? 8 : 4;
}

// what both impact calls check first, in this order
int impact_check(const char* call, csim_ensemble* e, csim_obs_network* n, const double* weight) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_REQUIRE(n, "null network");
    CSIM_REQUIRE(n->e == e, "the network belongs to another ensemble");
    CSIM_REQUIRE(weight, "null weight");
    if (!n->imp.valid)
        return fail(CSIM_ERR_STATE, std::string(call) + ": the network has no capture (csim_obs_network_impact_capture)");
    CSIM_REQUIRE(interior_finite(weight, e->g.nx, e->g.ny), "every interior value of the weight must be finite");
    return CSIM_OK;
}

// and what both end with.  Args: ImpactArgs or ImpactGlobalArgs, of which the capture's part is filled in here;
// enqueue(a, out) stages the weight its own way, fills in the rest and launches the kernels that leave J in plan
// order's `out`.  Then J and the status snapshot come back, and the summary is made of them
template <class Args, class Enqueue>
int impact_run(const char* call, csim_ensemble* e, csim_obs_network* n, double* out_impact,
               csim_obs_impact_summary* summary, Enqueue&& enqueue) {
    csim_obs_network::Impact& x = n->imp;
    try {
        std::vector<double> J(n->nobs);
        std::vector<unsigned char> snap(n->nobs);
        Args a{};
        a.nobs = n->nobs, a.forecast = x.M, a.idx = n->args().idx;
        a.snap = buf_at<unsigned char>(x.aux.p, n->imp_snap());
        a.pert = x.pert.as(), a.dn = buf_at<double>(x.aux.p, n->imp_dn());
        double* out = buf_at<double>(x.aux.p, n->imp_out());
        CSIM_TRY(enqueue(a, out));
        CSIM_HIP(hipMemcpyAsync(J.data(), out, sizeof(double) * J.size(), hipMemcpyDeviceToHost, e->st));
        CSIM_HIP(hipMemcpyAsync(snap.data(), a.snap, snap.size(), hipMemcpyDeviceToHost, e->st));
        CSIM_HIP(hipStreamSynchronize(e->st));
        if (out_impact) std::copy(J.begin(), J.end(), out_impact);
        if (summary) {
            summary->used = summary->beneficial = 0;
            for (unsigned char s : snap) summary->used += s == CSIM_OBS_USED;
            // the chunks of csim_obs_cycle: T_c from +0 in input order, their running sum from +0 in chunk order
            double total = 0.0;
            for (int c0 = 0; c0 < n->nobs; c0 += OBS_CHUNK) {
                double T = 0.0;
                for (int o = c0; o < std::min(n->nobs, c0 + OBS_CHUNK); ++o) {
                    T = T + J[o];
                    summary->beneficial += J[o] < 0.0;
                }
                total = total + T;
            }
            summary->total = total;
        }
        return CSIM_OK;
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, std::string(call) + ": out of host memory");
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

int csim_ensemble_assimilate_network(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                     int record) {
    return csim_ensemble_assimilate_screened(e, n, inflation, truth_member, record, 0.0);
}

int csim_ensemble_assimilate_screened(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                      int record, double tol) {
    int M = 0, t = 0;
    CSIM_TRY(analysis_check(e, n, inflation, truth_member, record, tol, &M, &t));
    if (n->batches_m != M) {
        assim_batches(e->g.nx, e->g.ny, *n, assim_batch_size(M), &n->batches);
        n->batches_m = M;
    }
    Analysis x;
    CSIM_TRY(analysis_begin(e, n, M, t, record, tol, &x));
    CSIM_TRY(assim_enqueue(e, x.a, inflation, n->batches));
    return record ? analysis_record(e, n, x) : CSIM_OK;
}

int csim_ensemble_assimilate_local(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                   int record, double tol) {
    int M = 0, t = 0, lmax = 0;
    CSIM_TRY(analysis_check(e, n, inflation, truth_member, record, tol, &M, &t));
    const EnsGeom& g = e->g;
    CSIM_TRY(local_max(n, &lmax));
    if (lmax > CSIM_LOCAL_MAX_OBS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_local: more than CSIM_LOCAL_MAX_OBS observation "
                                          "windows over one cell");
    if (static_cast<long>(lmax) * M > CSIM_LOCAL_MAX_DOUBLES)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_local: the windows over one cell times the forecast "
                                          "members exceed CSIM_LOCAL_MAX_DOUBLES");
    const size_t doubles = static_cast<size_t>(n->nobs) * M;
    if (doubles > static_cast<size_t>(CSIM_LOCAL_MAX_PRIOR_DOUBLES))
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_local: nobs times the forecast members exceeds "
                                          "CSIM_LOCAL_MAX_PRIOR_DOUBLES");
    csim_obs_network::Local& x = n->loc;
    const int tile = local_tile(e);
    try {
        // the lookup for this tile, made and uploaded when the tile is another one than the last
        if (x.tiles.key != tile) {
            LocalTiles lt;
            if (!local_tiles_build(g.nx, g.ny, *n, tile, &lt))
                return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_local: the lookup exceeds 2^31 entries");
            CSIM_TRY(x.tiles.upload(lt.start, lt.pos, tile, e->st));
            x.ntx = lt.ntx, x.nty = lt.nty;
        }
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, "csim_ensemble_assimilate_local: out of host memory");
    }
    CSIM_TRY(x.prior.reserve(sizeof(double) * doubles, e->st));
    Analysis an;
    CSIM_TRY(analysis_begin(e, n, M, t, record, tol, &an));
    double* f = e->base(e->cur);
    if (inflation != 1.0) CSIM_HIP(ens_launch_assim_inflate(g, f, M, t, inflation - 1.0, e->st));
    LocalArgs l{};
    l.tile = x.tiles.key, l.ntx = x.ntx, l.nty = x.nty, l.lmax = lmax;
    l.pack = ens_local_pack(M, lmax, e->local.pack);
    l.cstart = x.tiles.cstart(), l.cpos = x.tiles.cpos();
    l.prior = x.prior.as();
    CSIM_HIP(ens_launch_local_prior(g, f, an.a, n->nobs, x.prior.as(), e->st));
    CSIM_HIP(ens_launch_local_update(g, f, an.a, l, e->st));
    return record ? analysis_record(e, n, an) : CSIM_OK;
}

int csim_ensemble_obs_gram(csim_ensemble* e, csim_obs_network* n, int truth_member, double* A, double* loglik,
                           long long* n_used) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_REQUIRE(n, "null network");
    CSIM_REQUIRE(n->e == e, "the network belongs to another ensemble");
    int M = 0, t = 0;
    CSIM_TRY(forecast_split(e->g.members, truth_member, &M, &t, 2, "the observation-space Gram matrix needs at least "
                            "two forecast members", ESPACE_MAX_MEMBERS,
                            "csim_ensemble_obs_gram: at most CSIM_ESPACE_MAX_MEMBERS forecast members"));
    if (!n->has_values)
        return fail(CSIM_ERR_STATE, "csim_ensemble_obs_gram: the network has no values yet "
                                    "(csim_obs_network_set_values or csim_obs_network_observe)");
    try {
        std::vector<double> out;
        long long used = 0;
        CSIM_TRY(obs_gram(e, n, M, t, n->masked ? n->at<unsigned char>(n->l.mask) : nullptr, 1, loglik != nullptr, &out,
                          &used));
        const size_t ma = static_cast<size_t>(M) + 1;
        if (A) std::copy(out.begin(), out.begin() + ma * ma, A);
        if (loglik) std::copy(out.begin() + ma * ma, out.begin() + ma * ma + M, loglik);
        if (n_used) *n_used = used;
        return CSIM_OK;
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, "csim_ensemble_obs_gram: out of host memory");
    }
}

int csim_ensemble_assimilate_etkf(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                  int record, double tol) {
    int M = 0, t = 0;
    CSIM_TRY(etkf_check(e, n, inflation, truth_member, record, tol, &M, &t));
    try {
        const size_t m = static_cast<size_t>(M), ma = m + 1;
        std::vector<double> out, W(m * m), wbar(m), gamma(m);
        long long used = 0;
        double dfs = 0.0;
        Analysis x;
        e->espace.etkf_valid = false, e->espace.etkf_pending = false;
        CSIM_TRY(analysis_begin(e, n, M, t, record, tol, &x));
        CSIM_TRY(obs_gram(e, n, M, t, x.screen ? x.s.status : nullptr, CSIM_OBS_USED, false, &out, &used));
        for (size_t k = 0; k < ma * ma; ++k)
            if (!std::isfinite(out[k])) return fail(CSIM_ERR_STATE, ETKF_NONFINITE_TEXT);
        CSIM_TRY(csim_etkf_weights(M, out.data(), inflation, W.data(), wbar.data(), gamma.data(), &dfs, nullptr));
        // nothing to assimilate and nothing to inflate: W would be the identity up to rounding, the members keep their bits
        if (used != 0 || inflation != 1.0) CSIM_TRY(csim_ensemble_transform(e, truth_member, 1, W.data(), wbar.data()));
        csim_ensemble::Espace& s = e->espace;
        s.etkf_gamma.swap(gamma);
        s.etkf_used = used, s.etkf_chi2 = out[ma * ma - 1], s.etkf_dfs = dfs, s.etkf_valid = true;
        s.etkf_sweeps = 0, s.etkf_status = CSIM_EIGEN_OK;
        return record ? analysis_record(e, n, x) : CSIM_OK;
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, "csim_ensemble_assimilate_etkf: out of host memory");
    }
}

int csim_ensemble_assimilate_etkf_device(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                         int record, double tol) {
    int M = 0, t = 0;
    CSIM_TRY(etkf_check(e, n, inflation, truth_member, record, tol, &M, &t));
    CSIM_REQUIRE(e->g.slab <= 0x7fffffffL, "grid too large for the ensemble-space kernels");
    csim_ensemble::Espace& s = e->espace;
    if (!eigen_device_form(M, s.eigen_form))
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_etkf_device: the eigen_form that is set does not "
                                          "admit this many forecast members");
    const size_t m = static_cast<size_t>(M);
    const EtkfLayout l(M);
    s.etkf_valid = false, s.etkf_pending = false;
    CSIM_TRY(s.w.reserve(sizeof(double) * (m * m + m), e->st));
    CSIM_TRY(s.eig.reserve(sizeof(double) * l.doubles, e->st));
    Analysis x;
    CSIM_TRY(analysis_begin(e, n, M, t, record, tol, &x));
    CSIM_TRY(obs_gram_enqueue(e, n, M, t, x.screen ? x.s.status : nullptr, CSIM_OBS_USED, false));
    double* d = s.eig.as();
    int* info = reinterpret_cast<int*>(d + l.info);
    auto* rec = reinterpret_cast<EtkfRecord*>(d + l.rec);
    CSIM_HIP(ens_launch_sym_eigen(M, 1, s.gram.as(), M + 1, 0, d + l.work, d + l.lam, d + l.V, info, s.eigen_form,
                                  e->st));
    CSIM_HIP(ens_launch_etkf_weights(M, s.gram.as(), d + l.lam, d + l.V, info, inflation, s.w.as(), s.w.as() + m * m,
                                     rec, d + l.gamma, e->st));
    // as csim_ensemble_transform: only interior cells of the forecast members in the current buffer are written; the
    // kernel returns at once where the record says that there is nothing to do or that A is not finite
    CSIM_HIP(ens_launch_transform(e->g, e->base(e->cur), M, t, true, s.w.as(), s.w.as() + m * m, s.project_form, e->st,
                                  &rec->status));
    s.etkf_pending = true, s.etkf_m = M;
    return record ? analysis_record(e, n, x) : CSIM_OK;
}

int csim_ensemble_etkf_info2(csim_ensemble* e, long long* n_used, double* chi2, double* dfs, double* gamma,
                             int* n_gamma, int* sweeps, int* status) {
    CSIM_REQUIRE(e, "null ensemble");
    csim_ensemble::Espace& s = e->espace;
    if (s.etkf_pending) {
        // the record of the device path: wait for the stream and fetch it, once
        const EtkfLayout l(s.etkf_m);
        try {
            std::vector<double> got(4 + static_cast<size_t>(s.etkf_m));
            CSIM_HIP(hipMemcpyAsync(got.data(), s.eig.as() + l.rec, sizeof(double) * got.size(), hipMemcpyDeviceToHost,
                                    e->st));
            CSIM_HIP(hipStreamSynchronize(e->st));
            EtkfRecord rec;
            std::memcpy(&rec, got.data(), sizeof rec);
            s.etkf_pending = false;
            s.etkf_sweeps = rec.sweeps;
            s.etkf_status = rec.status == ETKF_NONFINITE        ? CSIM_EIGEN_NONFINITE
                            : rec.status == ETKF_NOT_CONVERGED ? CSIM_EIGEN_NOT_CONVERGED
                                                               : CSIM_EIGEN_OK;
            if (rec.status == ETKF_NONFINITE) return fail(CSIM_ERR_STATE, ETKF_NONFINITE_TEXT);
            s.etkf_gamma.assign(got.begin() + 4, got.end());
            s.etkf_used = rec.n_used, s.etkf_chi2 = rec.chi2, s.etkf_dfs = rec.dfs, s.etkf_valid = true;
        } catch (const std::bad_alloc&) {
            return fail(CSIM_ERR_STATE, "csim_ensemble_etkf_info: out of host memory");
        }
    }
    if (!s.etkf_valid)
        return fail(CSIM_ERR_STATE, "csim_ensemble_etkf_info: the ensemble's last csim_ensemble_assimilate_etkf did not "
                                    "complete, or there was none");
    if (n_used) *n_used = s.etkf_used;
    if (chi2) *chi2 = s.etkf_chi2;
    if (dfs) *dfs = s.etkf_dfs;
    if (gamma) std::copy(s.etkf_gamma.begin(), s.etkf_gamma.end(), gamma);
    if (n_gamma) *n_gamma = static_cast<int>(s.etkf_gamma.size());
    if (sweeps) *sweeps = s.etkf_sweeps;
    if (status) *status = s.etkf_status;
    return CSIM_OK;
}

int csim_ensemble_etkf_info(const csim_ensemble* e, long long* n_used, double* chi2, double* dfs, double* gamma,
                            int* n_gamma) {
    // a pending record of the device path is fetched into the handle, which this older signature declares const
    return csim_ensemble_etkf_info2(const_cast<csim_ensemble*>(e), n_used, chi2, dfs, gamma, n_gamma, nullptr, nullptr);
}

int csim_ensemble_assimilate_letkf(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member, int record,
                                   double tol, int spacing) {
    int M = 0, t = 0;
    CSIM_TRY(analysis_check(e, n, inflation, truth_member, record, tol, &M, &t));
    CSIM_REQUIRE(spacing >= 1, "spacing must be >= 1");
    const EnsGeom& g = e->g;
    CSIM_REQUIRE(g.slab <= 0x7fffffffL, "grid too large for the ensemble-space kernels");
    if (M > ESPACE_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_letkf: at most CSIM_ESPACE_MAX_MEMBERS forecast "
                                          "members");
    const size_t doubles = static_cast<size_t>(n->nobs) * M;
    if (doubles > static_cast<size_t>(CSIM_LOCAL_MAX_PRIOR_DOUBLES))
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_letkf: nobs times the forecast members exceeds "
                                          "CSIM_LOCAL_MAX_PRIOR_DOUBLES");
    const int nax = letkf_axis_nodes(g.nx, spacing), nay = letkf_axis_nodes(g.ny, spacing);
    const long nodes = static_cast<long>(nax) * nay;
    if (nodes > CSIM_LETKF_MAX_NODES)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_letkf: more than CSIM_LETKF_MAX_NODES analysis nodes; "
                                          "take a larger spacing");
    const int eform = eigen_device_form(M, e->espace.eigen_form);
    if (!eform)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_letkf: the eigen_form that is set does not admit "
                                          "this many forecast members");
    // the limit is on the bytes that csim_letkf_plan reports; a forced eigen_form may keep more in global memory
    if (static_cast<long long>(letkf_layout(M, nodes, eigen_device_form(M, 0)).bytes) > CSIM_LETKF_MAX_BYTES)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_letkf: the node storage exceeds CSIM_LETKF_MAX_BYTES "
                                          "(csim_letkf_plan); take a larger spacing");
    const LetkfLayout l = letkf_layout(M, nodes, eform);
    csim_obs_network::Letkf& x = n->letkf;
    csim_ensemble::Letkf& s = e->letkf;
    try {
        // the lookup for this spacing, made and uploaded when the spacing is another one than the last
        if (x.nodes.key != spacing) {
            LetkfLookup lk;
            if (!letkf_lookup_build(g.nx, g.ny, *n, spacing, &lk))
                return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_letkf: the lookup exceeds 2^31 entries");
            CSIM_TRY(x.nodes.upload(lk.start, lk.pos, spacing, e->st));
        }
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, "csim_ensemble_assimilate_letkf: out of host memory");
    }
    CSIM_TRY(n->loc.prior.reserve(sizeof(double) * doubles, e->st));
    s.valid = false;  // from here on the last record is being overwritten (in stream order, after its readers)
    CSIM_TRY(s.buf.reserve(l.bytes, e->st));
    Analysis an;
    CSIM_TRY(analysis_begin(e, n, M, t, record, tol, &an));
    double* f = e->base(e->cur);
    if (inflation != 1.0) CSIM_HIP(ens_launch_assim_inflate(g, f, M, t, inflation - 1.0, e->st));
    CSIM_HIP(ens_launch_local_prior(g, f, an.a, n->nobs, n->loc.prior.as(), e->st));
    void* const d = s.buf.p;
    LetkfGramArgs ga{};
    ga.nax = nax, ga.nay = nay, ga.spacing = spacing;
    ga.cstart = x.nodes.cstart(), ga.cpos = x.nodes.cpos();
    ga.prior = n->loc.prior.as();
    ga.A = buf_at<double>(d, l.A), ga.count = buf_at<int>(d, l.count);
    CSIM_HIP(ens_launch_letkf_gram(g, an.a, ga, e->espace.obs_gram_form, e->st));
    CSIM_HIP(ens_launch_sym_eigen(M, static_cast<int>(nodes), ga.A, M + 1, static_cast<long>(M + 1) * (M + 1),
                                  buf_at<double>(d, l.work), buf_at<double>(d, l.lam), buf_at<double>(d, l.V),
                                  buf_at<int>(d, l.info), e->espace.eigen_form, e->st));
    CSIM_HIP(ens_launch_letkf_weights(M, static_cast<int>(nodes), ga.A, buf_at<double>(d, l.lam), buf_at<double>(d, l.V),
                                      buf_at<int>(d, l.info), ga.count, buf_at<double>(d, l.W), buf_at<double>(d, l.wbar),
                                      buf_at<double>(d, l.dfs), buf_at<int>(d, l.sweeps), buf_at<int>(d, l.status),
                                      e->st));
    LetkfCellArgs ca{};
    ca.nax = nax, ca.nay = nay, ca.spacing = spacing;
    ca.W = buf_at<double>(d, l.W), ca.wbar = buf_at<double>(d, l.wbar), ca.status = buf_at<int>(d, l.status);
    CSIM_HIP(ens_launch_letkf_cells(g, f, M, t, ca, s.form, e->st));
    s.valid = true, s.l = l, s.nax = nax, s.nay = nay;
    return record ? analysis_record(e, n, an) : CSIM_OK;
}

int csim_ensemble_letkf_info(csim_ensemble* e, int* nax, int* nay, double* dfs, int* count, int* sweeps, int* status) {
    CSIM_REQUIRE(e, "null ensemble");
    csim_ensemble::Letkf& s = e->letkf;
    if (!s.valid)
        return fail(CSIM_ERR_STATE, "csim_ensemble_letkf_info: the ensemble has had no csim_ensemble_assimilate_letkf");
    const size_t nodes = static_cast<size_t>(s.nax) * s.nay;
    if (nax) *nax = s.nax;
    if (nay) *nay = s.nay;
    try {
        std::vector<int> st(nodes);
        if (dfs)
            CSIM_HIP(hipMemcpyAsync(dfs, buf_at<char>(s.buf.p, s.l.dfs), sizeof(double) * nodes, hipMemcpyDeviceToHost, e->st));
        if (count)
            CSIM_HIP(hipMemcpyAsync(count, buf_at<char>(s.buf.p, s.l.count), sizeof(int) * nodes, hipMemcpyDeviceToHost, e->st));
        if (sweeps)
            CSIM_HIP(hipMemcpyAsync(sweeps, buf_at<char>(s.buf.p, s.l.sweeps), sizeof(int) * nodes, hipMemcpyDeviceToHost, e->st));
        CSIM_HIP(hipMemcpyAsync(st.data(), buf_at<char>(s.buf.p, s.l.status), sizeof(int) * nodes, hipMemcpyDeviceToHost, e->st));
        CSIM_HIP(hipStreamSynchronize(e->st));
        if (status) std::copy(st.begin(), st.end(), status);
        for (int v : st)
            if (v == CSIM_LETKF_NONFINITE)
                return fail(CSIM_ERR_STATE, "csim_ensemble_letkf_info: the Gram matrix of a node has a non-finite entry; "
                                            "the cells that only such nodes feed are unchanged");
        return CSIM_OK;
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, "csim_ensemble_letkf_info: out of host memory");
    }
}

int csim_obs_network_local_info(csim_obs_network* n, int* max_local) {
    CSIM_REQUIRE(n, "null network");
    CSIM_REQUIRE(max_local, "null argument");
    return local_max(n, max_local);
}

int csim_obs_network_impact_capture(csim_obs_network* n, int truth_member) {
    CSIM_REQUIRE(n, "null network");
    csim_ensemble* e = n->e;
    const EnsGeom& g = e->g;
    int M = 0, t = 0;
    CSIM_TRY(forecast_split(g.members, truth_member, &M, &t, 2, "the impact needs at least two forecast members",
                            ASSIM_MAX_MEMBERS, "csim_obs_network_impact_capture: at most 1024 forecast members"));
    CSIM_REQUIRE(g.slab <= 0x7fffffffL, "grid too large for the impact");
    const size_t doubles = static_cast<size_t>(n->nobs) * M;
    if (doubles > static_cast<size_t>(CSIM_IMPACT_MAX_DOUBLES))
        return fail(CSIM_ERR_UNSUPPORTED, "csim_obs_network_impact_capture: nobs times the forecast members exceeds "
                                          "CSIM_IMPACT_MAX_DOUBLES");
    if (!n->has_diag || !n->last_recorded)
        return fail(CSIM_ERR_STATE, "csim_obs_network_impact_capture: the network's last analysis was not recorded "
                                    "(csim_ensemble_assimilate_network with record = 1)");
    csim_obs_network::Impact& x = n->imp;
    // a buffer that has to grow is replaced after the stream has drained, and the old capture goes with it
    if (sizeof(double) * doubles > x.pert.cap || n->imp_bytes() > x.aux.cap) x.valid = false;
    CSIM_TRY(x.pert.reserve(sizeof(double) * doubles, e->st));
    CSIM_TRY(x.aux.reserve(n->imp_bytes(), e->st));
    x.valid = false;  // from here on the last capture is being overwritten (in stream order, after its readers)
    const ObsArgs oa = n->args();
    const AssimArgs a = assim_args(M, t, *n, n->at<double>(n->l.rho), {oa.i, oa.j, oa.idx, oa.y, oa.r}, nullptr, nullptr,
                                   nullptr, oa.tstart, oa.toff, oa.tw, n->tmax);
    const ImpactCapture c{oa.bg, n->screened ? n->at<unsigned char>(n->l.status) : nullptr, x.pert.as(),
                          buf_at<double>(x.aux.p, n->imp_dn()), buf_at<unsigned char>(x.aux.p, n->imp_snap())};
    CSIM_HIP(ens_launch_impact_capture(g, e->base(e->cur), a, n->nobs, c, e->st));
    x.valid = true, x.M = M, x.t = t;
    return CSIM_OK;
}

int csim_ensemble_obs_impact(csim_ensemble* e, csim_obs_network* n, const double* weight, double* out_impact,
                             csim_obs_impact_summary* summary) {
    CSIM_TRY(impact_check("csim_ensemble_obs_impact", e, n, weight));
    auto enqueue = [&](ImpactArgs& a, double* out) -> int {
        const EnsGeom& g = e->g;
        csim_obs_network::Impact& x = n->imp;
        const size_t nx2 = static_cast<size_t>(g.nx) + 2, cells = stats_cells(e);
        // the interior of the weight, +0 on the ghost ring, copied before any kernel runs
        void* staged = nullptr;
        CSIM_TRY(x.wstage.acquire(sizeof(double) * cells, &staged));
        auto* hw = static_cast<double*>(staged);
        std::fill(hw, hw + cells, 0.0);
        for (int j = 1; j <= g.ny; ++j) std::copy(weight + j * nx2 + 1, weight + j * nx2 + 1 + g.nx, hw + j * nx2 + 1);
        CSIM_TRY(x.w.reserve(sizeof(double) * cells, e->st));
        CSIM_TRY(x.wstage.send(x.w.p, sizeof(double) * cells, e->st));
        const ObsArgs oa = n->args();
        a.truth_member = x.t, a.lx = n->lx, a.ly = n->ly;
        a.rho = n->at<double>(n->l.rho), a.i = oa.i, a.j = oa.j, a.w = x.w.as();
        CSIM_HIP(ens_launch_obs_impact(g, e->base(e->cur), a, out, e->st));
        return CSIM_OK;
    };
    return impact_run<ImpactArgs>("csim_ensemble_obs_impact", e, n, out_impact, summary, enqueue);
}

int csim_ensemble_obs_impact_global(csim_ensemble* e, csim_obs_network* n, const double* weight, double* out_impact,
                                    csim_obs_impact_summary* summary) {
    CSIM_TRY(impact_check("csim_ensemble_obs_impact_global", e, n, weight));
    if (n->imp.M > ESPACE_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_obs_impact_global: at most CSIM_ESPACE_MAX_MEMBERS forecast "
                                          "members");
    auto enqueue = [&](ImpactGlobalArgs& a, double* out) -> int {
        // g = dot(centered, the weight) stays on the device between the fold and the impact kernel
        CSIM_TRY(dot_stage_fields(e, 1, weight));
        CSIM_TRY(dot_enqueue(e, n->imp.M, n->imp.t, true, 1));
        a.g = e->espace.dot_out.as();
        CSIM_HIP(ens_launch_obs_impact_global(a, out, e->st));
        return CSIM_OK;
    };
    return impact_run<ImpactGlobalArgs>("csim_ensemble_obs_impact_global", e, n, out_impact, summary, enqueue);
}

int csim_obs_impact_global_value(int M, const double* a, const double* g, double dn, double* J) {
    CSIM_REQUIRE(a && g && J, "null argument");
    CSIM_REQUIRE(M >= 2, "M must be >= 2");
    double c = 0.0;
    for (int k = 0; k < M; ++k) c = c + a[k] * g[k];
    const double S = c / static_cast<double>(M - 1);
    *J = dn * S;
    return CSIM_OK;
}

int csim_obs_impact_fold(const double* u, long n, double* S) {
    CSIM_REQUIRE(S, "null argument");
    CSIM_REQUIRE(n >= 0 && (n == 0 || u), "n must be >= 0, with that many values");
    *S = impact_fold(u, n);
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
