// include/climate/ensemble.hpp — RAII handle of the batched stepper (csim_ensemble_* in include/csim.h): B members of
// one grid shape, each with its own field and (D, dt, vx, vy), advanced together on one GPU.  Every member ends bit
// for bit where a single-rank climate::Stepper run with its own parameters would.  Calls only the C ABI.
#pragma once
#include <algorithm>
#include <cstddef>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "csim.h"

namespace climate {

// per-cell statistics over the members, each member_size() values in the reference layout (see csim_ensemble_stats)
struct EnsembleStats {
    std::vector<double> mean, var, min, max;
};

// per-cell quantiles and exceedance probabilities over the members (see csim_ensemble_quantiles): q holds one field of
// member_size() values per level, exceed one per threshold, one after the other
struct EnsembleQuantiles {
    std::vector<double> q, exceed;
};

// verification against a truth (see csim_ensemble_verify): crps one field of member_size() values, brier one per
// threshold, rank_hist M + 1 bins (M forecast members), scores over the non-NaN interior cells
struct EnsembleVerification {
    std::vector<double> crps, brier;
    std::vector<unsigned long long> rank_hist;
    csim_verify_scores scores;
};

// neighbourhood and probability verification (see csim_ensemble_verify_spatial): the integer tables of the device
// (table: thresholds x (forecast + 1) x 2, nbh: thresholds x scales x 3), the non-NaN and NaN interior cells, and
// what csim_verify_spatial_finish makes of them: the scores and the ROC points (thresholds x (forecast + 1) each)
struct SpatialVerification {
    std::vector<unsigned long long> table, nbh;
    unsigned long long cells = 0, nan_cells = 0;
    std::size_t thresholds = 0, scales = 0, forecast = 0;
    csim_spatial_scores scores{};
    std::vector<double> hit_rate, false_alarm;
};

// host-only: whether M forecast members on nx x ny cells with half-widths up to half_max are inside the overflow bound
// of csim_verify_spatial_limit; other errors throw
inline bool verify_spatial_limit(int M, int nx, int ny, int half_max) {
    const int rc = csim_verify_spatial_limit(M, nx, ny, half_max);
    if (rc != CSIM_OK && rc != CSIM_ERR_UNSUPPORTED) throw std::runtime_error(std::string("csim: ") + csim_last_error());
    return rc == CSIM_OK;
}

// an analysis (see csim_ensemble_assimilate): the plan's level count and, per observation in input order, the forecast
// mean and variance at its cell at its turn and the analysis mean and variance there after all observations
struct EnsembleAnalysis {
    int nlevels = 0;
    std::vector<double> prior_mean, prior_var, post_mean, post_var;
};

// what an observation network holds per observation, in input order (see csim_obs_network_fetch); truth is empty
// unless the values were observed from a member, the diagnostics are empty before the first recorded analysis
struct ObsValues {
    std::vector<double> y, truth, bg_mean, bg_var, post_mean, post_var;
};

// the taps of linear observations (see csim_obs_network_create_linear): observation o observes
// sum_s w[s] x(i[o] + di[s], j[o] + dj[s]) over s = start[o] .. start[o + 1] - 1; i, j are the anchors
struct ObsTaps {
    std::vector<int> i, j, start{0}, di, dj;
    std::vector<double> w;
    std::size_t size() const { return i.size(); }
};

// the forecast impact of a network's observations (see csim_ensemble_obs_impact): J_o per observation in input order,
// J_o < 0: the observation reduced the forecast error, and the summary
struct ObsImpact {
    std::vector<double> impact;
    csim_obs_impact_summary summary{};
};

// eigenvalues (descending) and vectors (n x n row-major, column r belongs to lambda[r]) of a symmetric matrix
struct SymEigen {
    std::vector<double> lambda, V;
    int sweeps = 0;
};
// cyclic Jacobi on the n x n row-major symmetric matrix A, host only (see csim_sym_eigen_ordered); order
// CSIM_EIGEN_ROWS or CSIM_EIGEN_ROUND_ROBIN, the order of the device solver
inline SymEigen sym_eigen(const std::vector<double>& A, int n, int order = CSIM_EIGEN_ROWS) {
    if (n < 0 || A.size() != static_cast<std::size_t>(n) * static_cast<std::size_t>(n))
        throw std::invalid_argument("sym_eigen: array size");
    SymEigen e;
    e.lambda.resize(static_cast<std::size_t>(n));
    e.V.resize(A.size());
    if (csim_sym_eigen_ordered(n, A.data(), order, e.lambda.data(), e.V.data(), &e.sweeps) != CSIM_OK)
        throw std::runtime_error(std::string("csim: ") + csim_last_error());
    return e;
}
// `batch` symmetric matrices, n x n row-major one after the other, on the GPU in the round-robin order, one workgroup
// each (see csim_sym_eigen_batch_gpu); status per matrix: CSIM_EIGEN_OK, _NONFINITE (NaN results) or _NOT_CONVERGED
struct SymEigenBatch {
    std::vector<double> lambda, V;
    std::vector<int> sweeps, status;
};
inline SymEigenBatch sym_eigen_batch(const std::vector<double>& A, int n, int batch, int form = 0) {
    if (n < 0 || batch < 0 ||
        A.size() != static_cast<std::size_t>(batch) * static_cast<std::size_t>(n) * static_cast<std::size_t>(n))
        throw std::invalid_argument("sym_eigen_batch: array size");
    SymEigenBatch e;
    e.lambda.resize(static_cast<std::size_t>(batch) * static_cast<std::size_t>(n));
    e.V.resize(A.size());
    e.sweeps.resize(static_cast<std::size_t>(batch)), e.status.resize(static_cast<std::size_t>(batch));
    if (csim_sym_eigen_batch_gpu(n, batch, A.data(), e.lambda.data(), e.V.data(), e.sweeps.data(), e.status.data(),
                                 form) != CSIM_OK)
        throw std::runtime_error(std::string("csim: ") + csim_last_error());
    return e;
}

// the observation-space Gram matrix of a network (see csim_ensemble_obs_gram): A (M + 1) x (M + 1) row-major, loglik M
// values (empty when not asked for), and the observations used
struct ObsGram {
    std::vector<double> A, loglik;
    long long n_used = 0;
};
// the ETKF's weights (see csim_etkf_weights): Ensemble::transform(W, wbar) is the analysis
struct EtkfWeights {
    std::vector<double> W, wbar, gamma;
    double dfs = 0.0;
    int sweeps = 0;
};
// from the (M + 1) x (M + 1) matrix of Ensemble::obs_gram(), host only, on sym_eigen in the given order
inline EtkfWeights etkf_weights(const std::vector<double>& A, int M, double inflation = 1.0,
                                int order = CSIM_EIGEN_ROWS) {
    if (M < 0 || A.size() != static_cast<std::size_t>(M + 1) * static_cast<std::size_t>(M + 1))
        throw std::invalid_argument("etkf_weights: array size");
    EtkfWeights w;
    const std::size_t m = static_cast<std::size_t>(M);
    w.W.resize(m * m), w.wbar.resize(m), w.gamma.resize(m);
    if (csim_etkf_weights_ordered(M, A.data(), inflation, order, w.W.data(), w.wbar.data(), w.gamma.data(), &w.dfs,
                                  &w.sweeps) != CSIM_OK)
        throw std::runtime_error(std::string("csim: ") + csim_last_error());
    return w;
}
// what an ETKF analysis found (see csim_ensemble_etkf_info)
struct EtkfAnalysis {
    long long n_used = 0;
    double chi2 = 0.0, dfs = 0.0;
    std::vector<double> gamma;
    int sweeps = 0, status = CSIM_EIGEN_OK;  // of the device eigensolver, after assimilate_etkf_device (else 0)
};

// the lattice of analysis nodes of Ensemble::assimilate_letkf (see csim_letkf_nodes): nay x nax nodes, node (a, b) at the
// interior cell (xi[a], yj[b]) with index b nax + a.  Host only
struct LetkfNodes {
    int nax = 0, nay = 0;
    std::vector<int> xi, yj;
};
inline LetkfNodes letkf_nodes(int nx, int ny, int spacing) {
    LetkfNodes n;
    if (csim_letkf_nodes(nx, ny, spacing, &n.nax, &n.nay, nullptr, nullptr) != CSIM_OK)
        throw std::runtime_error(std::string("csim: ") + csim_last_error());
    n.xi.resize(n.nax), n.yj.resize(n.nay);
    if (csim_letkf_nodes(nx, ny, spacing, nullptr, nullptr, n.xi.data(), n.yj.data()) != CSIM_OK)
        throw std::runtime_error(std::string("csim: ") + csim_last_error());
    return n;
}
// the four nodes of the interior cell (i, j) and the weights with which their analyses are blended there (see
// csim_letkf_blend).  Host only
struct LetkfBlend {
    int node[4] = {0, 0, 0, 0};
    double beta[4] = {0.0, 0.0, 0.0, 0.0};
};
inline LetkfBlend letkf_blend(int nx, int ny, int spacing, int i, int j) {
    LetkfBlend b;
    if (csim_letkf_blend(nx, ny, spacing, i, j, b.node, b.beta) != CSIM_OK)
        throw std::runtime_error(std::string("csim: ") + csim_last_error());
    return b;
}
// what the nodes of an LETKF found (see csim_ensemble_letkf_info): nay x nax values each, row-major
struct LetkfInfo {
    int nax = 0, nay = 0;
    std::vector<double> dfs;
    std::vector<int> count, sweeps, status;  // status: CSIM_LETKF_*
};

// the leading modes of an ensemble's spread (see csim_ensemble_eofs): lambda and variance = lambda / (M - 1) per mode,
// pcs M x n_modes row-major, patterns n_modes dense fields (empty when not asked for)
struct EnsembleEOFs {
    std::vector<double> lambda, variance, pcs, patterns;
    int n_valid = 0;
};

class Ensemble;

// observations that live on the device (csim_obs_network_*): planned once, their values drawn on the GPU from a
// member or set from the host, read by Ensemble::assimilate(ObsNetwork&, ...) without staging.  Move-only; made by
// Ensemble::obs_network().  The library destroys the networks of an ensemble with it; the ensemble then empties the
// handle this class shares with it, so a network that outlives its ensemble is safe to destroy or move, and every
// other call on it throws.
class ObsNetwork {
public:
    ~ObsNetwork() { close(); }
    ObsNetwork(ObsNetwork&&) noexcept = default;
    ObsNetwork& operator=(ObsNetwork&& o) noexcept {
        if (this != &o) {
            close();
            slot_ = std::move(o.slot_), nobs_ = o.nobs_;
        }
        return *this;
    }
    ObsNetwork(const ObsNetwork&) = delete;
    ObsNetwork& operator=(const ObsNetwork&) = delete;

    std::size_t size() const { return nobs_; }
    // taps of all observations of a linear network, 0 for point observations
    int taps() const {
        int n = 0;
        check(csim_obs_network_taps(handle(), &n));
        return n;
    }
    int levels() const {
        int nl = 0;
        check(csim_obs_network_info(handle(), nullptr, &nl, nullptr, nullptr));
        return nl;
    }
    // one finite value per observation, copied before the call returns; enqueued
    void set_values(const std::vector<double>& y) {
        if (y.size() != nobs_) throw std::invalid_argument("obs network: one value per observation");
        check(csim_obs_network_set_values(handle(), y.data()));
    }
    // the values from member source_member, with noise plus sqrt(r) times the deviates of (seed, draw); enqueued
    void observe(int source_member, unsigned long long seed, unsigned draw = 0, bool noise = true) {
        check(csim_obs_network_observe(handle(), source_member, seed, draw, noise ? 1 : 0));
    }
    // the same for the observations of one time slot, the others keep their values (see csim_obs_network_observe_slot)
    void observe_slot(int slot, int source_member, unsigned long long seed, unsigned draw = 0, bool noise = true) {
        check(csim_obs_network_observe_slot(handle(), slot, source_member, seed, draw, noise ? 1 : 0));
    }
    // the time slot of every observation, 0 .. CSIM_OBS_MAX_SLOTS - 1; forgets which slots are held; enqueued
    void set_slots(const std::vector<int>& slot) {
        if (slot.size() != nobs_) throw std::invalid_argument("obs network: one slot per observation");
        check(csim_obs_network_set_slots(handle(), slot.data()));
    }
    // keeps h_k of every forecast member for the observations of the slot (-1: all) from the members as they are now,
    // for Ensemble::assimilate_etkf_held() at the end of the window (see csim_obs_network_hold); t as in
    // Ensemble::assimilate.  Enqueued
    void hold(int slot = -1, int t = -1) { check(csim_obs_network_hold(handle(), slot, t)); }
    // waits for the ensemble's stream: the held rows, size() x M row-major in input order; after a held analysis the
    // transformed rows (see csim_obs_network_held)
    std::vector<double> held() {
        int M = 0;
        check(csim_obs_network_held(handle(), nullptr, &M, nullptr));
        std::vector<double> H(nobs_ * static_cast<std::size_t>(M));
        check(csim_obs_network_held(handle(), H.data(), nullptr, nullptr));
        return H;
    }
    // waits for the ensemble's stream
    ObsValues fetch(bool truth = false, bool diagnostics = false) {
        ObsValues v;
        v.y.resize(nobs_);
        if (truth) v.truth.resize(nobs_);
        if (diagnostics)
            for (std::vector<double>* a : {&v.bg_mean, &v.bg_var, &v.post_mean, &v.post_var}) a->resize(nobs_);
        check(csim_obs_network_fetch(handle(), v.y.data(), truth ? v.truth.data() : nullptr,
                                     diagnostics ? v.bg_mean.data() : nullptr, diagnostics ? v.bg_var.data() : nullptr,
                                     diagnostics ? v.post_mean.data() : nullptr,
                                     diagnostics ? v.post_var.data() : nullptr));
        return v;
    }
    // waits for the ensemble's stream: the recorded analyses, oldest first
    std::vector<csim_obs_cycle> log() {
        int k = 0;
        check(csim_obs_network_log(handle(), 0, nullptr, &k));
        std::vector<csim_obs_cycle> out(static_cast<std::size_t>(k));
        check(csim_obs_network_log(handle(), k, out.data(), &k));
        return out;
    }
    void log_reset() { check(csim_obs_network_log_reset(handle())); }
    // screening (see csim_obs_network_set_active): one byte per observation, 1 active, 0 a missing report; copied
    // before the call returns, enqueued, and kept until it is replaced
    void set_active(const std::vector<unsigned char>& active) {
        if (active.size() != nobs_) throw std::invalid_argument("obs network: one mask byte per observation");
        check(csim_obs_network_set_active(handle(), active.data()));
    }
    void set_all_active() { check(csim_obs_network_set_active(handle(), nullptr)); }
    // waits for the ensemble's stream: CSIM_OBS_USED / _INACTIVE / _REJECTED per observation for the last analysis
    std::vector<unsigned char> status() {
        std::vector<unsigned char> s(nobs_);
        check(csim_obs_network_status(handle(), s.data()));
        return s;
    }
    // waits for the ensemble's stream: the used / inactive / rejected counts of the recorded analyses, oldest first
    std::vector<csim_obs_screen_cycle> screen_log() {
        int k = 0;
        check(csim_obs_network_screen_log(handle(), 0, nullptr, &k));
        std::vector<csim_obs_screen_cycle> out(static_cast<std::size_t>(k));
        check(csim_obs_network_screen_log(handle(), k, out.data(), &k));
        return out;
    }
    // keeps what Ensemble::obs_impact() needs of the last analysis, which must be a recorded one (see
    // csim_obs_network_impact_capture); t as in Ensemble::assimilate.  Enqueued; valid across run() until the next capture
    void impact_capture(int t = -1) { check(csim_obs_network_impact_capture(handle(), t)); }
    // the most window rectangles of the network over one cell, which Ensemble::assimilate_local() holds against
    // CSIM_LOCAL_MAX_OBS (see csim_obs_network_local_info)
    int local_info() {
        int most = 0;
        check(csim_obs_network_local_info(handle(), &most));
        return most;
    }

private:
    friend class Ensemble;
    // the handle, shared with the ensemble that made it: null once either side has destroyed the network
    struct Slot {
        csim_obs_network* h = nullptr;
    };
    ObsNetwork(std::shared_ptr<Slot> slot, std::size_t nobs) : slot_(std::move(slot)), nobs_(nobs) {}
    csim_obs_network* handle() const { return slot_ ? slot_->h : nullptr; }  // null: the library refuses the call
    void close() {
        if (slot_ && slot_->h) csim_obs_network_destroy(slot_->h);
        if (slot_) slot_->h = nullptr;
        slot_.reset();
    }
    static void check(int rc) {
        if (rc != CSIM_OK) throw std::runtime_error(std::string("csim: ") + csim_last_error());
    }
    std::shared_ptr<Slot> slot_;
    std::size_t nobs_ = 0;
};

class Ensemble {
public:
    Ensemble(int members, int nx, int ny, double dx, double dy, const int bc[4], double bc_value = 0.0)
        : members_(members), nx_(nx), ny_(ny) {
        check(csim_ensemble_create(members, nx, ny, 1, dx, dy, bc, bc_value, &h_));
    }
    ~Ensemble() {
        for (auto& slot : nets_) slot->h = nullptr;  // csim_ensemble_destroy destroys the networks that are alive
        csim_ensemble_destroy(h_);
    }
    Ensemble(const Ensemble&) = delete;
    Ensemble& operator=(const Ensemble&) = delete;

    int members() const { return members_; }
    std::size_t member_size() const { return static_cast<std::size_t>(nx_ + 2) * static_cast<std::size_t>(ny_ + 2); }

    // reference layout with the ghost ring, (ny+2) x (nx+2) per member; the _all forms: members x that, contiguous
    void upload(int member, const std::vector<double>& a) { check(csim_ensemble_upload(h_, member, sized(a, 1))); }
    void upload_all(const std::vector<double>& a) { check(csim_ensemble_upload_all(h_, sized(a, members_))); }
    std::vector<double> download(int member) {
        std::vector<double> a(member_size());
        check(csim_ensemble_download(h_, member, a.data()));
        return a;
    }
    std::vector<double> download_all() {
        std::vector<double> a(member_size() * members_);
        check(csim_ensemble_download_all(h_, a.data()));
        return a;
    }
    void init_gaussian(int member, double A, double sigma_frac, double xc_frac, double yc_frac) {
        check(csim_ensemble_init_gaussian(h_, member, A, sigma_frac, xc_frac, yc_frac));
    }
    // one value per member each (dt as given: clamp with csim_safe_dt)
    void set_physics(const std::vector<double>& D, const std::vector<double>& dt, const std::vector<double>& vx,
                     const std::vector<double>& vy) {
        const std::size_t n = static_cast<std::size_t>(members_);
        if (D.size() != n || dt.size() != n || vx.size() != n || vy.size() != n)
            throw std::invalid_argument("set_physics: one value per member");
        check(csim_ensemble_set_physics(h_, D.data(), dt.data(), vx.data(), vy.data()));
    }
    void run(int nsteps) { check(csim_ensemble_run(h_, nsteps)); }
    void sync() { check(csim_ensemble_sync(h_)); }
    std::vector<unsigned long long> checksums() {
        std::vector<unsigned long long> c(static_cast<std::size_t>(members_));
        check(csim_ensemble_checksum(h_, c.data()));
        return c;
    }
    std::vector<double> minmax() {  // min, max per member (ghosts included)
        std::vector<double> m(2 * static_cast<std::size_t>(members_));
        check(csim_ensemble_minmax(h_, m.data()));
        return m;
    }
    std::vector<double> sums() {
        std::vector<double> s(static_cast<std::size_t>(members_));
        check(csim_ensemble_sum(h_, s.data()));
        return s;
    }
    EnsembleStats stats(int ddof = 1) {
        EnsembleStats r;
        for (std::vector<double>* v : {&r.mean, &r.var, &r.min, &r.max}) v->resize(member_size());
        check(csim_ensemble_stats(h_, ddof, r.mean.data(), r.var.data(), r.min.data(), r.max.data()));
        return r;
    }
    // captured after everything enqueued so far; run() may be called before stats_wait()
    void stats_begin(int ddof = 1) { check(csim_ensemble_stats_begin(h_, ddof)); }
    // host pointers of member_size() values each, valid until the next stats_begin() or destruction
    struct StatsView {
        const double *mean, *var, *min, *max;
    };
    StatsView stats_wait() {
        StatsView v{};
        check(csim_ensemble_stats_wait(h_, &v.mean, &v.var, &v.min, &v.max));
        return v;
    }
    EnsembleQuantiles quantiles(const std::vector<double>& q, const std::vector<double>& thresholds = {}) {
        EnsembleQuantiles r;
        r.q.resize(q.size() * member_size());
        r.exceed.resize(thresholds.size() * member_size());
        check(csim_ensemble_quantiles(h_, static_cast<int>(q.size()), q.data(), static_cast<int>(thresholds.size()),
                                      thresholds.data(), r.q.data(), r.exceed.data()));
        return r;
    }
    // captured after everything enqueued so far; run() may be called before quantiles_wait()
    void quantiles_begin(const std::vector<double>& q, const std::vector<double>& thresholds = {}) {
        check(csim_ensemble_quantiles_begin(h_, static_cast<int>(q.size()), q.data(),
                                            static_cast<int>(thresholds.size()), thresholds.data()));
        q_levels_ = q.size();
        q_thresholds_ = thresholds.size();
    }
    // host pointers of levels (thresholds) x member_size() values, valid until the next quantiles_begin() or destruction
    struct QuantilesView {
        const double *q, *exceed;
        std::size_t levels, thresholds;
    };
    QuantilesView quantiles_wait() {
        QuantilesView v{nullptr, nullptr, q_levels_, q_thresholds_};
        check(csim_ensemble_quantiles_wait(h_, &v.q, &v.exceed));
        return v;
    }
    // the members against a host truth field (member_size() values)
    EnsembleVerification verify(const std::vector<double>& truth, const std::vector<double>& thresholds = {},
                                bool fair = false) {
        return verify_any(sized(truth, 1), -1, members_, thresholds, fair);
    }
    // member t against the other members, in their order
    EnsembleVerification verify_member(int t, const std::vector<double>& thresholds = {}, bool fair = false) {
        return verify_any(nullptr, t, members_ - 1, thresholds, fair);
    }
    // captured after everything enqueued so far (a host truth is copied before the call returns); run() may be called
    // before verify_wait()
    void verify_begin(const std::vector<double>& truth, const std::vector<double>& thresholds = {}, bool fair = false) {
        check(csim_ensemble_verify_begin(h_, sized(truth, 1), -1, fair ? 1 : 0, static_cast<int>(thresholds.size()),
                                         thresholds.data()));
        v_forecast_ = static_cast<std::size_t>(members_);
        v_thresholds_ = thresholds.size();
    }
    void verify_member_begin(int t, const std::vector<double>& thresholds = {}, bool fair = false) {
        check(csim_ensemble_verify_begin(h_, nullptr, t, fair ? 1 : 0, static_cast<int>(thresholds.size()),
                                         thresholds.data()));
        v_forecast_ = static_cast<std::size_t>(members_ - 1);
        v_thresholds_ = thresholds.size();
    }
    // host pointers (crps: member_size(), brier: thresholds x member_size(), rank_hist: bins values), valid until the
    // next verify_begin() or destruction, and the finished scores
    struct VerifyView {
        const double *crps, *brier;
        const unsigned long long* rank_hist;
        std::size_t thresholds, bins;
        csim_verify_scores scores;
    };
    VerifyView verify_wait() {
        VerifyView v{nullptr, nullptr, nullptr, v_thresholds_, v_forecast_ + 1, {}};
        check(csim_ensemble_verify_wait(h_, &v.crps, &v.brier, &v.rank_hist, &v.scores));
        return v;
    }
    // neighbourhood and probability verification of the members against a host truth field (member_size() values) or
    // of the other members against member t: contingency tables and window sums as exact integers from the device,
    // finished into Brier decomposition, ROC and Fractions Skill Score on the host (see csim_ensemble_verify_spatial)
    SpatialVerification verify_spatial(const std::vector<double>& truth, const std::vector<double>& thresholds,
                                       const std::vector<int>& half_widths = {}) {
        return spatial_any(sized(truth, 1), -1, members_, thresholds, half_widths);
    }
    SpatialVerification verify_spatial_member(int t, const std::vector<double>& thresholds,
                                              const std::vector<int>& half_widths = {}) {
        return spatial_any(nullptr, t, members_ - 1, thresholds, half_widths);
    }
    // captured after everything enqueued so far, with a capture of its own: run(), verify_begin(), stats_begin() and
    // quantiles_begin() may follow before verify_spatial_wait(), which copies the tables and finishes the scores
    void verify_spatial_begin(const std::vector<double>& truth, const std::vector<double>& thresholds,
                              const std::vector<int>& half_widths = {}) {
        check(csim_ensemble_verify_spatial_begin(h_, sized(truth, 1), -1, static_cast<int>(thresholds.size()),
                                                 thresholds.data(), static_cast<int>(half_widths.size()),
                                                 half_widths.data(), 0));
        s_forecast_ = members_, s_thresholds_ = thresholds.size(), s_scales_ = half_widths.size();
    }
    void verify_spatial_member_begin(int t, const std::vector<double>& thresholds,
                                     const std::vector<int>& half_widths = {}) {
        check(csim_ensemble_verify_spatial_begin(h_, nullptr, t, static_cast<int>(thresholds.size()), thresholds.data(),
                                                 static_cast<int>(half_widths.size()), half_widths.data(), 0));
        s_forecast_ = members_ - 1, s_thresholds_ = thresholds.size(), s_scales_ = half_widths.size();
    }
    SpatialVerification verify_spatial_wait() {
        const unsigned long long *table = nullptr, *nbh = nullptr;
        SpatialVerification r;
        check(csim_ensemble_verify_spatial_wait(h_, &table, &nbh, nullptr, nullptr, &r.cells, &r.nan_cells));
        shape(r, s_forecast_, s_thresholds_, s_scales_);
        std::copy(table, table + r.table.size(), r.table.begin());
        std::copy(nbh, nbh + r.nbh.size(), r.nbh.begin());
        finish(r);
        return r;
    }
    // serial EnSRF analysis with point observations (i[o], j[o], y[o], r[o]), Gaspari-Cohn length loc; t = -1: all
    // members are the forecast, else member t is left alone.  Synchronous, with the diagnostics
    EnsembleAnalysis assimilate(const std::vector<int>& i, const std::vector<int>& j, const std::vector<double>& y,
                                const std::vector<double>& r, double loc, double inflation = 1.0, int t = -1,
                                bool ordered = false) {
        const std::size_t n = obs_size(i, j, y, r);
        EnsembleAnalysis a;
        a.prior_mean.resize(n), a.prior_var.resize(n), a.post_mean.resize(n), a.post_var.resize(n);
        check(csim_ensemble_assimilate(h_, static_cast<int>(n), i.data(), j.data(), y.data(), r.data(), loc, inflation,
                                       t, ordered ? 1 : 0, a.prior_mean.data(), a.prior_var.data(), a.post_mean.data(),
                                       a.post_var.data(), &a.nlevels));
        return a;
    }
    // the same without diagnostics: enqueued on the ensemble's stream (the observations are copied before it returns),
    // so that run() follows without a host wait; returns the level count
    int assimilate_enqueue(const std::vector<int>& i, const std::vector<int>& j, const std::vector<double>& y,
                           const std::vector<double>& r, double loc, double inflation = 1.0, int t = -1,
                           bool ordered = false) {
        int nl = 0;
        check(csim_ensemble_assimilate(h_, static_cast<int>(obs_size(i, j, y, r)), i.data(), j.data(), y.data(),
                                       r.data(), loc, inflation, t, ordered ? 1 : 0, nullptr, nullptr, nullptr,
                                       nullptr, &nl));
        return nl;
    }
    // an observation network on the device: cells, error variances, localisation and plan made once; log_cycles: room
    // for that many recorded analyses (see csim_obs_network_create)
    ObsNetwork obs_network(const std::vector<int>& i, const std::vector<int>& j, const std::vector<double>& r,
                           double loc, bool ordered = false, int log_cycles = 0) {
        if (j.size() != i.size() || r.size() != i.size())
            throw std::invalid_argument("ensemble: observation arrays of different sizes");
        nets_.erase(std::remove_if(nets_.begin(), nets_.end(), [](const auto& slot) { return !slot->h; }), nets_.end());
        auto slot = std::make_shared<ObsNetwork::Slot>();
        check(csim_obs_network_create(h_, static_cast<int>(i.size()), i.data(), j.data(), r.data(), loc,
                                      ordered ? 1 : 0, log_cycles, &slot->h));
        nets_.push_back(slot);
        return ObsNetwork(std::move(slot), i.size());
    }
    // the same for linear observations (see csim_obs_network_create_linear): taps from bilinear_taps() / box_taps() or
    // the caller's own
    ObsNetwork obs_network(const ObsTaps& t, const std::vector<double>& r, double loc, bool ordered = false,
                           int log_cycles = 0) {
        if (t.j.size() != t.i.size() || r.size() != t.i.size() || t.start.size() != t.i.size() + 1 ||
            t.start.back() < 0 || t.di.size() != t.w.size() || t.dj.size() != t.w.size() ||
            t.w.size() < static_cast<std::size_t>(t.start.back()))
            throw std::invalid_argument("ensemble: observation arrays of different sizes");
        nets_.erase(std::remove_if(nets_.begin(), nets_.end(), [](const auto& slot) { return !slot->h; }), nets_.end());
        auto slot = std::make_shared<ObsNetwork::Slot>();
        check(csim_obs_network_create_linear(h_, static_cast<int>(t.i.size()), t.i.data(), t.j.data(), t.start.data(),
                                             t.di.data(), t.dj.data(), t.w.data(), r.data(), loc, ordered ? 1 : 0,
                                             log_cycles, &slot->h));
        nets_.push_back(slot);
        return ObsNetwork(std::move(slot), t.i.size());
    }
    // host-only builders of taps: bilinear interpolation to the positions (x, y) in cell-index units, 1 <= x <= nx,
    // 1 <= y <= ny (csim_obs_taps_bilinear), and the means over (2a+1) x (2b+1) boxes around the cells (i, j), clipped
    // to the interior (csim_obs_taps_box)
    static ObsTaps bilinear_taps(int nx, int ny, const std::vector<double>& x, const std::vector<double>& y) {
        if (x.size() != y.size()) throw std::invalid_argument("ensemble: observation arrays of different sizes");
        ObsTaps t;
        for (std::size_t o = 0; o < x.size(); ++o) {
            int i = 0, j = 0, di[4], dj[4];
            double w[4];
            check(csim_obs_taps_bilinear(nx, ny, x[o], y[o], &i, &j, di, dj, w));
            t.i.push_back(i), t.j.push_back(j);
            t.di.insert(t.di.end(), di, di + 4), t.dj.insert(t.dj.end(), dj, dj + 4), t.w.insert(t.w.end(), w, w + 4);
            t.start.push_back(static_cast<int>(t.w.size()));
        }
        return t;
    }
    static ObsTaps box_taps(int nx, int ny, const std::vector<int>& i, const std::vector<int>& j, int a, int b) {
        if (i.size() != j.size()) throw std::invalid_argument("ensemble: observation arrays of different sizes");
        ObsTaps t;
        for (std::size_t o = 0; o < i.size(); ++o) {
            int n = 0, di[CSIM_OBS_MAX_TAPS], dj[CSIM_OBS_MAX_TAPS];
            double w[CSIM_OBS_MAX_TAPS];
            check(csim_obs_taps_box(nx, ny, i[o], j[o], a, b, &n, di, dj, w));
            t.i.push_back(i[o]), t.j.push_back(j[o]);
            t.di.insert(t.di.end(), di, di + n), t.dj.insert(t.dj.end(), dj, dj + n), t.w.insert(t.w.end(), w, w + n);
            t.start.push_back(static_cast<int>(t.w.size()));
        }
        return t;
    }
    // the analysis with the network's observations, always enqueued; record: also append the cycle's innovation
    // statistics to the network's log on the device (see csim_ensemble_assimilate_network).  screen_tol > 0: the
    // background check of csim_ensemble_assimilate_screened, which rejects an observation with
    // (y - hb)^2 > screen_tol^2 (vb + r); the network's active mask acts either way
    void assimilate(ObsNetwork& net, double inflation = 1.0, int t = -1, bool record = false, double screen_tol = 0.0) {
        check(csim_ensemble_assimilate_screened(h_, net.handle(), inflation, t, record ? 1 : 0, screen_tol));
    }
    // the local analysis with the network's observations, always enqueued: every cell from all used observations near
    // it, R-localised, in input order, one pass whatever the network (see csim_ensemble_assimilate_local); the
    // arguments as for assimilate(ObsNetwork&, ...)
    void assimilate_local(ObsNetwork& net, double inflation = 1.0, int t = -1, bool record = false,
                          double screen_tol = 0.0) {
        check(csim_ensemble_assimilate_local(h_, net.handle(), inflation, t, record ? 1 : 0, screen_tol));
    }
    // the LETKF with the network's observations, always enqueued: ensemble-space weights from the used observations near
    // each node of the lattice letkf_nodes(nx, ny, spacing), R-localised, blended to the cells between the nodes;
    // spacing 1 is the full LETKF (see csim_ensemble_assimilate_letkf); the other arguments as for assimilate_local
    void assimilate_letkf(ObsNetwork& net, double inflation = 1.0, int t = -1, bool record = false,
                          double screen_tol = 0.0, int spacing = 8) {
        check(csim_ensemble_assimilate_letkf(h_, net.handle(), inflation, t, record ? 1 : 0, screen_tol, spacing));
    }
    // what the nodes of the last assimilate_letkf found; waits for the stream, and throws when a node's Gram matrix was
    // not finite (see csim_ensemble_letkf_info)
    LetkfInfo letkf_info() {
        LetkfInfo r;
        const int rc = csim_ensemble_letkf_info(h_, &r.nax, &r.nay, nullptr, nullptr, nullptr, nullptr);
        if (r.nax == 0) check(rc);  // there was no LETKF
        const std::size_t n = static_cast<std::size_t>(r.nax) * r.nay;
        r.dfs.resize(n), r.count.resize(n), r.sweeps.resize(n), r.status.resize(n);
        check(csim_ensemble_letkf_info(h_, nullptr, nullptr, r.dfs.data(), r.count.data(), r.sweeps.data(),
                                       r.status.data()));
        return r;
    }
    // the observation-space Gram matrix of the forecast members over the network's active observations, and with loglik
    // each member's sum of squared normalised departures; synchronous, writes nothing of the network (see
    // csim_ensemble_obs_gram)
    ObsGram obs_gram(ObsNetwork& net, int t = -1, bool loglik = false) {
        const std::size_t M = forecast(t);
        ObsGram g;
        g.A.resize((M + 1) * (M + 1));
        if (loglik) g.loglik.resize(M);
        check(csim_ensemble_obs_gram(h_, net.handle(), t, g.A.data(), loglik ? g.loglik.data() : nullptr, &g.n_used));
        return g;
    }
    // the same from the rows that the network holds (ObsNetwork::hold) instead of the current members; the members and
    // the truth member are the hold's (see csim_ensemble_obs_gram_held)
    ObsGram obs_gram_held(ObsNetwork& net, bool loglik = false) {
        int m = 0;
        check(csim_obs_network_held(net.handle(), nullptr, &m, nullptr));
        const std::size_t M = static_cast<std::size_t>(m);
        ObsGram g;
        g.A.resize((M + 1) * (M + 1));
        if (loglik) g.loglik.resize(M);
        check(csim_ensemble_obs_gram_held(h_, net.handle(), g.A.data(), loglik ? g.loglik.data() : nullptr, &g.n_used));
        return g;
    }
    // the global ETKF analysis with the network's observations: obs_gram() over the used ones, etkf_weights() and
    // transform() composed in the library; waits for the Gram matrix, the transform is enqueued (see
    // csim_ensemble_assimilate_etkf); the arguments as for assimilate(ObsNetwork&, ...)
    EtkfAnalysis assimilate_etkf(ObsNetwork& net, double inflation = 1.0, int t = -1, bool record = false,
                                 double screen_tol = 0.0) {
        check(csim_ensemble_assimilate_etkf(h_, net.handle(), inflation, t, record ? 1 : 0, screen_tol));
        EtkfAnalysis r;
        r.gamma.resize(forecast(t));
        check(csim_ensemble_etkf_info(h_, &r.n_used, &r.chi2, &r.dfs, r.gamma.data(), nullptr));
        return r;
    }
    // the same analysis with the eigensolver and the weights on the GPU, in the round-robin order: no copy and no wait,
    // without record the call only enqueues (see csim_ensemble_assimilate_etkf_device); etkf_info(t) tells what it found
    void assimilate_etkf_device(ObsNetwork& net, double inflation = 1.0, int t = -1, bool record = false,
                                double screen_tol = 0.0) {
        check(csim_ensemble_assimilate_etkf_device(h_, net.handle(), inflation, t, record ? 1 : 0, screen_tol));
    }
    // the 4D form of either: the weights from the rows that the network holds from its observations' own times, applied
    // to the members and to the rows; ends the window (see csim_ensemble_assimilate_etkf_held).  etkf_info(t) tells what
    // it found
    void assimilate_etkf_held(ObsNetwork& net, double inflation = 1.0, int t = -1, bool record = false,
                              double screen_tol = 0.0, bool device = false) {
        check(csim_ensemble_assimilate_etkf_held(h_, net.handle(), inflation, t, record ? 1 : 0, screen_tol,
                                                 device ? 1 : 0));
    }
    // what the last ETKF analysis found; after assimilate_etkf_device it waits for the stream first, and throws when
    // the Gram matrix was not finite (the members are then unchanged; see csim_ensemble_etkf_info2)
    EtkfAnalysis etkf_info(int t = -1) {
        EtkfAnalysis r;
        r.gamma.resize(forecast(t));
        check(csim_ensemble_etkf_info2(h_, &r.n_used, &r.chi2, &r.dfs, r.gamma.data(), nullptr, &r.sweeps, &r.status));
        return r;
    }
    // the forecast impact of every observation of net's captured analysis on the error of the current state (EFSOI, see
    // csim_ensemble_obs_impact); weight = C (e_a + e_b), member_size() values of which the interior is read.  Synchronous
    ObsImpact obs_impact(ObsNetwork& net, const std::vector<double>& weight) {
        return obs_impact_by(csim_ensemble_obs_impact, net, weight);
    }
    // the same without localisation, for a capture made after a global analysis (assimilate_etkf, either path): one read
    // of the members whatever the network (see csim_ensemble_obs_impact_global).  Synchronous
    ObsImpact obs_impact_global(ObsNetwork& net, const std::vector<double>& weight) {
        return obs_impact_by(csim_ensemble_obs_impact_global, net, weight);
    }
    // adds sigma times a seeded Gaussian random field of correlation length corr_len to the interior of every forecast
    // member (t = -1: all members, else member t is left alone); enqueued on the ensemble's stream, so that run() follows
    // without a host wait (see csim_ensemble_perturb)
    void perturb(double sigma, double corr_len, unsigned long long seed, unsigned draw = 0, bool centered = false,
                 int t = -1) {
        check(csim_ensemble_perturb(h_, seed, draw, sigma, corr_len, centered ? 1 : 0, t));
    }
    // relaxation inflation (see csim_ensemble_relax), mode CSIM_RELAX_SPREAD (RTPS) or CSIM_RELAX_PERT (RTPP); t as in
    // assimilate.  prior_capture() keeps what relax() needs of the forecast, before the analysis; relax() after the
    // analysis pulls its perturbations back towards the forecast ones.  Both are enqueued on the ensemble's stream, so
    // that prior_capture(); assimilate_enqueue(); relax(); run() needs no host wait
    void prior_capture(int mode, int t = -1) { check(csim_ensemble_prior_capture(h_, mode, t)); }
    void relax(int mode, double alpha, int t = -1) { check(csim_ensemble_relax(h_, mode, alpha, t, nullptr)); }
    // RTPS, synchronous: the factor f of every cell (member_size() values, +0 on the ghost ring)
    std::vector<double> relax_factor(double alpha, int t = -1) {
        std::vector<double> f(member_size());
        check(csim_ensemble_relax(h_, CSIM_RELAX_SPREAD, alpha, t, f.data()));
        return f;
    }
    // ensemble space (see csim_ensemble_gram): M forecast members, all of them or, with t >= 0, all but member t.
    // The M x M Gram matrix of the perturbations from the per-cell mean (centered) or of the members, row-major
    std::vector<double> gram(int t = -1, bool centered = true) {
        const std::size_t M = forecast(t);
        std::vector<double> G(M * M);
        check(csim_ensemble_gram(h_, t, centered ? 1 : 0, G.data()));
        return G;
    }
    // K dense fields out_r = sum_k p_k W[k K + r], W is M x K row-major
    std::vector<double> project(const std::vector<double>& W, int K, int t = -1, bool centered = true) {
        if (K < 0 || W.size() != forecast(t) * static_cast<std::size_t>(K))
            throw std::invalid_argument("ensemble: W must be M x K");
        std::vector<double> out(member_size() * static_cast<std::size_t>(K));
        check(csim_ensemble_project(h_, t, centered ? 1 : 0, K, W.data(), out.data()));
        return out;
    }
    // the adjoint of project: out[k K + r] = sum over the interior of p_k f_r, M x K row-major; fields holds K dense
    // fields, member_size() values each, of which the interior is read (see csim_ensemble_dot).  Synchronous
    std::vector<double> dot(const std::vector<double>& fields, int K, int t = -1, bool centered = true) {
        if (K < 0 || fields.size() != member_size() * static_cast<std::size_t>(K))
            throw std::invalid_argument("ensemble: fields must be K dense fields");
        std::vector<double> out(forecast(t) * static_cast<std::size_t>(K));
        check(csim_ensemble_dot(h_, t, centered ? 1 : 0, K, fields.data(), out.data()));
        return out;
    }
    // the forecast members replaced on the interior by a linear combination of them, W is M x M row-major and wbar
    // (centered only) M values or empty; enqueued without waiting, W and wbar may be reused at once
    void transform(const std::vector<double>& W, const std::vector<double>& wbar = {}, int t = -1,
                   bool centered = true) {
        const std::size_t M = forecast(t);
        if (W.size() != M * M || (!wbar.empty() && wbar.size() != M))
            throw std::invalid_argument("ensemble: W must be M x M and wbar M values");
        check(csim_ensemble_transform(h_, t, centered ? 1 : 0, W.data(), wbar.empty() ? nullptr : wbar.data()));
    }
    EnsembleEOFs eofs(int n_modes, int t = -1, bool patterns = true) {
        const std::size_t M = forecast(t), K = static_cast<std::size_t>(n_modes > 0 ? n_modes : 0);
        EnsembleEOFs r;
        r.lambda.resize(K), r.pcs.resize(M * K);
        if (patterns) r.patterns.resize(K * member_size());
        check(csim_ensemble_eofs(h_, t, n_modes, r.lambda.data(), r.pcs.data(), patterns ? r.patterns.data() : nullptr,
                                 &r.n_valid));
        for (double l : r.lambda) r.variance.push_back(l / static_cast<double>(M - 1));
        return r;
    }
    void set_option(const char* key, long value) { check(csim_ensemble_set_option(h_, key, value)); }
    long get_option(const char* key) const {
        long v = 0;
        check(csim_ensemble_get_option(h_, key, &v));
        return v;
    }

private:
    static void check(int rc) {
        if (rc != CSIM_OK) throw std::runtime_error(std::string("csim: ") + csim_last_error());
    }
    std::size_t forecast(int t) const { return static_cast<std::size_t>(members_ - (t >= 0 ? 1 : 0)); }
    const double* sized(const std::vector<double>& a, int n) const {
        if (a.size() != member_size() * static_cast<std::size_t>(n)) throw std::invalid_argument("ensemble: array size");
        return a.data();
    }
    ObsImpact obs_impact_by(decltype(&csim_ensemble_obs_impact) call, ObsNetwork& net, const std::vector<double>& weight) {
        ObsImpact r;
        r.impact.resize(net.size());
        check(call(h_, net.handle(), sized(weight, 1), r.impact.data(), &r.summary));
        return r;
    }
    EnsembleVerification verify_any(const double* truth, int t, int forecast, const std::vector<double>& thresholds,
                                    bool fair) {
        EnsembleVerification r{};
        r.crps.resize(member_size());
        r.brier.resize(thresholds.size() * member_size());
        r.rank_hist.resize(static_cast<std::size_t>(forecast > 0 ? forecast : 0) + 1);
        check(csim_ensemble_verify(h_, truth, t, fair ? 1 : 0, static_cast<int>(thresholds.size()), thresholds.data(),
                                   r.crps.data(), r.brier.data(), r.rank_hist.data(), &r.scores));
        return r;
    }
    static void shape(SpatialVerification& r, int forecast, std::size_t nt, std::size_t ns) {
        r.forecast = static_cast<std::size_t>(forecast > 0 ? forecast : 0);
        r.thresholds = nt, r.scales = ns;
        r.table.assign(nt * (r.forecast + 1) * 2, 0);
        r.nbh.assign(nt * ns * 3, 0);
        r.hit_rate.assign(nt * (r.forecast + 1), 0.0);
        r.false_alarm.assign(nt * (r.forecast + 1), 0.0);
    }
    static void finish(SpatialVerification& r) {
        check(csim_verify_spatial_finish(static_cast<int>(r.forecast), static_cast<int>(r.thresholds),
                                         static_cast<int>(r.scales), r.table.data(), r.nbh.data(), r.cells, r.nan_cells,
                                         &r.scores, r.hit_rate.data(), r.false_alarm.data()));
    }
    SpatialVerification spatial_any(const double* truth, int t, int forecast, const std::vector<double>& thresholds,
                                    const std::vector<int>& half_widths) {
        SpatialVerification r;
        shape(r, forecast, thresholds.size(), half_widths.size());
        check(csim_ensemble_verify_spatial(h_, truth, t, static_cast<int>(thresholds.size()), thresholds.data(),
                                           static_cast<int>(half_widths.size()), half_widths.data(), r.table.data(),
                                           r.nbh.data(), nullptr, nullptr, &r.cells, &r.nan_cells));
        finish(r);
        return r;
    }
    static std::size_t obs_size(const std::vector<int>& i, const std::vector<int>& j, const std::vector<double>& y,
                                const std::vector<double>& r) {
        if (j.size() != i.size() || y.size() != i.size() || r.size() != i.size())
            throw std::invalid_argument("ensemble: observation arrays of different sizes");
        return i.size();
    }
    csim_ensemble* h_ = nullptr;
    std::vector<std::shared_ptr<ObsNetwork::Slot>> nets_;  // the handles of the networks made here that are alive
    int members_, nx_, ny_;
    std::size_t q_levels_ = 0, q_thresholds_ = 0;  // of the last quantiles_begin()
    std::size_t v_forecast_ = 0, v_thresholds_ = 0;  // of the last verify_begin()
    int s_forecast_ = 0;                             // of the last verify_spatial_begin()
    std::size_t s_thresholds_ = 0, s_scales_ = 0;
};

}  // namespace climate
