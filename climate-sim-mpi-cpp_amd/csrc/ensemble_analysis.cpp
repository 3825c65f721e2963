// ensemble_analysis.cpp — the analyses that run on an observation network (obs_network.hpp; the network itself is
// ensemble_obs.cpp): the analysis only points an AssimArgs into the network's buffer and enqueues its launches.
// Five analyses share the checks, the screening and the recording (analysis_check, analysis_begin, analysis_record)
// and differ in what runs between them:
//   serial (csim_ensemble_assimilate_network, _screened)  the launches of ensemble_da.cpp's assim_enqueue
//   local  (ensemble_local.hip)  the observation priors and a lookup per tile, storage of the network's own
//   ETKF   the observation-space Gram matrix of the used observations (csim_ensemble_obs_gram, ensemble_obsgram.hip,
//          which writes nothing of the network), csim_etkf_weights on the host, csim_ensemble_transform; or, _device,
//          the eigensolver and the weights of sym_eigen_device.hip with no host round trip
//   LETKF  (ensemble_letkf.hip)  the local analysis's priors, a Gram matrix per node of a lattice, the batched
//          eigensolver and weights, and a cell pass that interpolates the weights; a lookup per spacing
//   held ETKF  (csim_ensemble_assimilate_etkf_held, ensemble_held.hip)  either ETKF with h_k read from the rows that the
//          network holds from the observations' own times (csim_obs_network_hold) in place of the state: (hb, vb), A and
//          (ha, va) come from the rows, and the rows are transformed with the members
// Screening (csim_obs_network_set_active, csim_ensemble_assimilate_screened) is one k_obs_screen launch ahead of the
// analysis, whose kernels then skip what is not used.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "obs_network.hpp"
#include "sym_eigen.hpp"

using namespace csim;

namespace {

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
    double* rows = nullptr;  // a held analysis: the network's held rows for a.forecast members, which stand for the state
};

// (mean, variance) of h_k of every observation, 2 per input index: from the state, or from the rows of a held analysis
hipError_t analysis_mv(csim_ensemble* e, csim_obs_network* n, const Analysis& x, double* out) {
    if (x.rows) return ens_launch_held_mv(x.rows, n->nobs, x.a.forecast, x.oa.idx, out, e->st);
    return ens_launch_assim_post(e->g, x.f, x.a, n->nobs, out, e->st);
}

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
    if (record || check) CSIM_HIP(analysis_mv(e, n, *x, bg));
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
    n->hold.last = x->rows != nullptr;
    return CSIM_OK;
}

// the last launches of a recorded analysis: (ha, va) and the cycle's records
int analysis_record(csim_ensemble* e, csim_obs_network* n, const Analysis& x) {
    CSIM_HIP(analysis_mv(e, n, x, n->at<double>(n->l.post)));
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
// rows: the held rows to read h_k from (csim_ensemble_obs_gram_held); null: the gather from the current buffer
int obs_gram_enqueue(csim_ensemble* e, csim_obs_network* n, int M, int t, const unsigned char* flag, int used,
                     bool want_ll, const double* rows = nullptr) {
    csim_ensemble::Espace& x = e->espace;
    const ObsArgs oa = n->args();
    ObsGramArgs a{};
    a.nobs = n->nobs, a.forecast = M, a.truth_member = t;
    a.i = oa.i, a.j = oa.j, a.y = oa.y, a.sr = oa.sr;
    a.flag = flag, a.used = used;
    a.tstart = oa.tstart, a.toff = oa.toff, a.tw = oa.tw;
    a.rows = rows;
    const size_t ma = static_cast<size_t>(M) + 1, doubles = ma * ma + M + 1;
    CSIM_TRY(x.partial.reserve(sizeof(double) * ens_obs_gram_partial_doubles(M, n->nobs), e->st));
    CSIM_TRY(x.gram.reserve(sizeof(double) * doubles, e->st));
    CSIM_HIP(ens_launch_obs_gram(e->g, e->base(e->cur), a, want_ll, x.partial.as(), x.gram.as(), x.obs_gram_form, e->st));
    return CSIM_OK;
}

int obs_gram(csim_ensemble* e, csim_obs_network* n, int M, int t, const unsigned char* flag, int used, bool want_ll,
             std::vector<double>* out, long long* n_used, const double* rows = nullptr) {
    csim_ensemble::Espace& x = e->espace;
    const size_t ma = static_cast<size_t>(M) + 1, doubles = ma * ma + M + 1;
    CSIM_TRY(obs_gram_enqueue(e, n, M, t, flag, used, want_ll, rows));
    out->resize(doubles);
    CSIM_HIP(hipMemcpyAsync(out->data(), x.gram.p, sizeof(double) * doubles, hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    static_assert(sizeof(long long) == sizeof(double), "the count travels behind loglik");
    std::memcpy(n_used, out->data() + ma * ma + M, sizeof(long long));
    return CSIM_OK;
}

// the state checks of a held analysis, after the analysis's own: every slot that occurs is held, for these members
int held_check(const csim_obs_network* n, int M, int t) {
    const csim_obs_network::Held& h = n->hold;
    if (!h.M || !h.all_held())
        return fail(CSIM_ERR_STATE, "csim_ensemble_assimilate_etkf_held: not every slot that occurs has been held since "
                                    "the last held analysis (csim_obs_network_hold)");
    if (h.M != M || h.t != t)
        return fail(CSIM_ERR_STATE, "csim_ensemble_assimilate_etkf_held: the rows were held with another truth_member");
    return CSIM_OK;
}

// a held analysis ends the window: no slot counts as held, the transformed rows stay until the next hold
void held_done(csim_obs_network* n) { n->hold.held = 0, n->hold.done = true; }

// csim_ensemble_assimilate_etkf, and with held csim_ensemble_assimilate_etkf_held(device = 0)
int etkf_host(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member, int record, double tol,
              bool held) {
    int M = 0, t = 0;
    CSIM_TRY(etkf_check(e, n, inflation, truth_member, record, tol, &M, &t));
    if (held) CSIM_TRY(held_check(n, M, t));
    try {
        const size_t m = static_cast<size_t>(M), ma = m + 1;
        std::vector<double> out, W(m * m), wbar(m), gamma(m);
        long long used = 0;
        double dfs = 0.0;
        Analysis x;
        if (held) x.rows = n->hold.rows.as();
        e->espace.etkf_valid = false, e->espace.etkf_pending = false;
        CSIM_TRY(analysis_begin(e, n, M, t, record, tol, &x));
        CSIM_TRY(obs_gram(e, n, M, t, x.screen ? x.s.status : nullptr, CSIM_OBS_USED, false, &out, &used, x.rows));
        for (size_t k = 0; k < ma * ma; ++k)
            if (!std::isfinite(out[k])) return fail(CSIM_ERR_STATE, ETKF_NONFINITE_TEXT);
        CSIM_TRY(csim_etkf_weights(M, out.data(), inflation, W.data(), wbar.data(), gamma.data(), &dfs, nullptr));
        // nothing to assimilate and nothing to inflate: W would be the identity up to rounding, the members keep their bits
        if (used != 0 || inflation != 1.0) {
            CSIM_TRY(csim_ensemble_transform(e, truth_member, 1, W.data(), wbar.data()));
            // the same (W, wbar), where the transform has put them, for the rows
            const double* w = e->espace.w.as();
            if (held) CSIM_HIP(ens_launch_held_transform(x.rows, n->nobs, M, w, w + m * m, e->st));
        }
        csim_ensemble::Espace& s = e->espace;
        s.etkf_gamma.swap(gamma);
        s.etkf_used = used, s.etkf_chi2 = out[ma * ma - 1], s.etkf_dfs = dfs, s.etkf_valid = true;
        s.etkf_sweeps = 0, s.etkf_status = CSIM_EIGEN_OK;
        if (held) held_done(n);
        return record ? analysis_record(e, n, x) : CSIM_OK;
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, "csim_ensemble_assimilate_etkf: out of host memory");
    }
}

// csim_ensemble_assimilate_etkf_device, and with held csim_ensemble_assimilate_etkf_held(device = 1)
int etkf_device(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member, int record, double tol,
                bool held) {
    int M = 0, t = 0;
    CSIM_TRY(etkf_check(e, n, inflation, truth_member, record, tol, &M, &t));
    CSIM_REQUIRE(e->g.slab <= 0x7fffffffL, "grid too large for the ensemble-space kernels");
    csim_ensemble::Espace& s = e->espace;
    if (!eigen_device_form(M, s.eigen_form))
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate_etkf_device: the eigen_form that is set does not "
                                          "admit this many forecast members");
    if (held) CSIM_TRY(held_check(n, M, t));
    const size_t m = static_cast<size_t>(M);
    const EtkfLayout l(M);
    s.etkf_valid = false, s.etkf_pending = false;
    CSIM_TRY(s.w.reserve(sizeof(double) * (m * m + m), e->st));
    CSIM_TRY(s.eig.reserve(sizeof(double) * l.doubles, e->st));
    Analysis x;
    if (held) x.rows = n->hold.rows.as();
    CSIM_TRY(analysis_begin(e, n, M, t, record, tol, &x));
    CSIM_TRY(obs_gram_enqueue(e, n, M, t, x.screen ? x.s.status : nullptr, CSIM_OBS_USED, false, x.rows));
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
    if (held) {
        CSIM_HIP(ens_launch_held_transform(x.rows, n->nobs, M, s.w.as(), s.w.as() + m * m, e->st, &rec->status));
        held_done(n);
    }
    s.etkf_pending = true, s.etkf_m = M;
    return record ? analysis_record(e, n, x) : CSIM_OK;
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

}  // namespace

extern "C" {

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
    return etkf_host(e, n, inflation, truth_member, record, tol, false);
}

int csim_ensemble_assimilate_etkf_device(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                         int record, double tol) {
    return etkf_device(e, n, inflation, truth_member, record, tol, false);
}

int csim_ensemble_obs_gram_held(csim_ensemble* e, csim_obs_network* n, double* A, double* loglik, long long* n_used) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_REQUIRE(n, "null network");
    CSIM_REQUIRE(n->e == e, "the network belongs to another ensemble");
    const csim_obs_network::Held& h = n->hold;
    if (!h.M || !h.all_held())
        return fail(CSIM_ERR_STATE, "csim_ensemble_obs_gram_held: not every slot that occurs has been held "
                                    "(csim_obs_network_hold)");
    if (!n->has_values)
        return fail(CSIM_ERR_STATE, "csim_ensemble_obs_gram_held: the network has no values yet");
    try {
        std::vector<double> out;
        long long used = 0;
        const int M = h.M;
        CSIM_TRY(obs_gram(e, n, M, h.t, n->masked ? n->at<unsigned char>(n->l.mask) : nullptr, 1, loglik != nullptr, &out,
                          &used, h.rows.as()));
        const size_t ma = static_cast<size_t>(M) + 1;
        if (A) std::copy(out.begin(), out.begin() + ma * ma, A);
        if (loglik) std::copy(out.begin() + ma * ma, out.begin() + ma * ma + M, loglik);
        if (n_used) *n_used = used;
        return CSIM_OK;
    } catch (const std::bad_alloc&) {
        return fail(CSIM_ERR_STATE, "csim_ensemble_obs_gram_held: out of host memory");
    }
}

int csim_ensemble_assimilate_etkf_held(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                       int record, double tol, int device) {
    CSIM_REQUIRE(device == 0 || device == 1, "device must be 0 or 1");
    return device ? etkf_device(e, n, inflation, truth_member, record, tol, true)
                  : etkf_host(e, n, inflation, truth_member, record, tol, true);
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

}  // extern "C"
