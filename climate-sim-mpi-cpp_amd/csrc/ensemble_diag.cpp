// ensemble_diag.cpp — the ensemble's diagnostics: per-cell statistics, quantiles and verification (kernels in
// ensemble_stats.hip, ensemble_quantiles.hip, ensemble_verify.hip).  Each has a synchronous entry point and a
// _begin / _wait pair that copies the result through a Capture of its own while the ensemble steps on.
#include <cmath>
#include <cstring>
#include <vector>

#include "ensemble_host.hpp"

using namespace csim;

namespace {

// checks ddof, prepares the capture, and enqueues the kernel on the ensemble's stream after everything enqueued so far
int stats_launch(csim_ensemble* e, int ddof, bool pinned) {
    CSIM_REQUIRE(ddof == 0 || ddof == 1, "ddof must be 0 or 1");
    CSIM_REQUIRE(e->g.members - ddof >= 1, "members - ddof must be >= 1");
    CSIM_REQUIRE(stats_cells(e) <= 0x7fffff00u, "grid too large for the statistics");
    // one size for every call: the buffers are made once and never replaced, so there is no stream to drain
    CSIM_TRY(e->stats.cap.prepare(4 * sizeof(double) * stats_cells(e), pinned, nullptr));
    CSIM_HIP(ens_launch_stats(e->g, e->base(e->cur), ddof, e->stats.cap.dev.as(), e->st));
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

// checks the arguments, prepares the capture, and enqueues the kernel on the ensemble's stream after everything
// enqueued so far
int quantiles_launch(csim_ensemble* e, int nq, const double* q, int nt, const double* thr, bool pinned) {
    CSIM_TRY(check_levels(nq, q));
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
    // nothing reads the buffers once the copy in flight and the kernels enqueued so far are done
    CSIM_TRY(e->quant.cap.prepare(sizeof(double) * (nq + nt) * stats_cells(e), pinned, e->st));
    CSIM_HIP(ens_launch_quantiles(e->g, e->base(e->cur), qa, e->quant.cap.dev.as(), e->st));
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

// checks the arguments, prepares the capture, stages a host truth, and enqueues the histogram's zeroing and the kernel
// on the ensemble's stream after everything enqueued so far.  *forecast, *blocks: of this call
int verify_launch(csim_ensemble* e, const double* truth, int truth_member, int fair, int nt, const double* thr,
                  bool pinned, int* forecast, int* blocks) {
    CSIM_REQUIRE((truth != nullptr) != (truth_member >= 0), "give exactly one truth: a host field or a member");
    int M = 0, t = 0;  // exactly one truth: a host field leaves all B members as the forecast, as no truth member does
    CSIM_TRY(forecast_split(e->g.members, truth_member, &M, &t));
    CSIM_REQUIRE(nt >= 0 && nt <= VERIFY_MAX_THRESHOLDS, "nt must be 0 .. 16");
    CSIM_REQUIRE(nt == 0 || thr, "null thresholds");
    CSIM_REQUIRE(fair == 0 || fair == 1, "fair must be 0 or 1");
    CSIM_REQUIRE(M >= 1, "no forecast members: a truth member needs at least two members");
    CSIM_REQUIRE(!fair || M >= 2, "the fair CRPS needs at least two forecast members");
    if (M > VERIFY_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_verify: at most 4096 forecast members (the largest sorting network)");
    CSIM_REQUIRE(stats_cells(e) * (VERIFY_MAX_THRESHOLDS + 1) <= 0x7fffff00u, "grid too large for the verification");
    const size_t cells = stats_cells(e);
    const int nb = ens_verify_blocks(e->g, M);
    const VerifyLayout l = verify_layout(M, nb, nt, cells);
    csim_ensemble::Verify& v = e->verify;
    CSIM_TRY(v.cap.prepare(sizeof(double) * l.total, pinned, e->st));
    VerifyArgs va{};
    va.forecast = M;
    va.truth_member = t;
    va.nt = nt;
    va.fair = fair;
    for (int k = 0; k < nt; ++k) va.thr[k] = thr[k];
    if (truth) {
        void* h = nullptr;
        CSIM_TRY(v.truth.reserve(sizeof(double) * cells));
        CSIM_TRY(v.stage.acquire(sizeof(double) * cells, &h));
        std::memcpy(h, truth, sizeof(double) * cells);
        CSIM_TRY(v.stage.send(v.truth.p, sizeof(double) * cells, e->st));
        va.truth = v.truth.as();
    }
    double* const d = v.cap.dev.as();
    VerifyOut o{};
    o.hist = reinterpret_cast<unsigned long long*>(d + l.hist);
    o.counts = reinterpret_cast<unsigned long long*>(d + l.counts);
    o.sums = d + l.sums;
    o.crps = d + l.crps;
    o.brier = d + l.brier;
    CSIM_HIP(hipMemsetAsync(o.hist, 0, sizeof(unsigned long long) * (M + 1), e->st));
    CSIM_HIP(ens_launch_verify(e->g, e->base(e->cur), va, o, e->st));
    *forecast = M;
    *blocks = nb;
    return CSIM_OK;
}

}  // namespace

extern "C" {

int csim_ensemble_stats(csim_ensemble* e, int ddof, double* mean, double* var, double* min, double* max) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_TRY(stats_launch(e, ddof, false));
    const size_t n = stats_cells(e);
    double* const outs[4] = {mean, var, min, max};
    for (int k = 0; k < 4; ++k)
        if (outs[k])
            CSIM_HIP(hipMemcpyAsync(outs[k], e->stats.cap.dev.as() + k * n, sizeof(double) * n, hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    return CSIM_OK;
}

int csim_ensemble_stats_begin(csim_ensemble* e, int ddof) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_TRY(stats_launch(e, ddof, true));
    return e->stats.cap.begin(4 * sizeof(double) * stats_cells(e), e->st);
}

int csim_ensemble_stats_wait(csim_ensemble* e, const double** mean, const double** var, const double** min,
                             const double** max) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_TRY(e->stats.cap.wait("no statistics in flight: csim_ensemble_stats_begin first"));
    const double** const outs[4] = {mean, var, min, max};
    for (int k = 0; k < 4; ++k)
        if (outs[k]) *outs[k] = e->stats.cap.host.as() + k * stats_cells(e);
    return CSIM_OK;
}

int csim_ensemble_quantiles(csim_ensemble* e, int nq, const double* q, int nt, const double* thr, double* out_q,
                            double* out_p) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_TRY(quantiles_launch(e, nq, q, nt, thr, false));
    const size_t n = stats_cells(e);
    const double* const d = e->quant.cap.dev.as();
    if (out_q && nq) CSIM_HIP(hipMemcpyAsync(out_q, d, sizeof(double) * nq * n, hipMemcpyDeviceToHost, e->st));
    if (out_p && nt) CSIM_HIP(hipMemcpyAsync(out_p, d + nq * n, sizeof(double) * nt * n, hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    return CSIM_OK;
}

int csim_ensemble_quantiles_begin(csim_ensemble* e, int nq, const double* q, int nt, const double* thr) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_TRY(quantiles_launch(e, nq, q, nt, thr, true));
    CSIM_TRY(e->quant.cap.begin(sizeof(double) * (nq + nt) * stats_cells(e), e->st));
    e->quant.nq = nq;
    return CSIM_OK;
}

int csim_ensemble_quantiles_wait(csim_ensemble* e, const double** out_q, const double** out_p) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_TRY(e->quant.cap.wait("no quantiles in flight: csim_ensemble_quantiles_begin first"));
    if (out_q) *out_q = e->quant.cap.host.as();
    if (out_p) *out_p = e->quant.cap.host.as() + e->quant.nq * stats_cells(e);
    return CSIM_OK;
}

int csim_ensemble_quantile_plan(int members, int nq, const double* q, int* lo, int* hi, double* gamma) {
    CSIM_REQUIRE(members >= 1, "members must be >= 1");
    CSIM_TRY(check_levels(nq, q));
    CSIM_REQUIRE(nq == 0 || (lo && hi && gamma), "null output");
    for (int k = 0; k < nq; ++k) quantile_plan(members, q[k], &lo[k], &hi[k], &gamma[k]);
    return CSIM_OK;
}

int csim_ensemble_verify(csim_ensemble* e, const double* truth, int truth_member, int fair, int nt, const double* thr,
                         double* out_crps, double* out_brier, unsigned long long* rank_hist,
                         csim_verify_scores* scores) {
    CSIM_REQUIRE(e, "null ensemble");
    int M = 0, nb = 0;
    CSIM_TRY(verify_launch(e, truth, truth_member, fair, nt, thr, false, &M, &nb));
    const size_t cells = stats_cells(e);
    const VerifyLayout l = verify_layout(M, nb, nt, cells);
    const double* const d = e->verify.cap.dev.as();
    std::vector<double> rec;
    if (out_crps) CSIM_HIP(hipMemcpyAsync(out_crps, d + l.crps, sizeof(double) * cells, hipMemcpyDeviceToHost, e->st));
    if (out_brier && nt)
        CSIM_HIP(hipMemcpyAsync(out_brier, d + l.brier, sizeof(double) * nt * cells, hipMemcpyDeviceToHost, e->st));
    if (rank_hist)
        CSIM_HIP(hipMemcpyAsync(rank_hist, d + l.hist, sizeof(unsigned long long) * (M + 1), hipMemcpyDeviceToHost, e->st));
    if (scores) {
        rec.resize(l.crps - l.counts);
        CSIM_HIP(hipMemcpyAsync(rec.data(), d + l.counts, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, e->st));
    }
    CSIM_HIP(hipStreamSynchronize(e->st));
    if (scores)
        verify_finish(reinterpret_cast<const unsigned long long*>(rec.data()), rec.data() + (l.sums - l.counts), nb, nt,
                      scores);
    return CSIM_OK;
}

// the scores are finished in _wait
int csim_ensemble_verify_begin(csim_ensemble* e, const double* truth, int truth_member, int fair, int nt,
                               const double* thr) {
    CSIM_REQUIRE(e, "null ensemble");
    int M = 0, nb = 0;
    CSIM_TRY(verify_launch(e, truth, truth_member, fair, nt, thr, true, &M, &nb));
    csim_ensemble::Verify& v = e->verify;
    CSIM_TRY(v.cap.begin(sizeof(double) * verify_layout(M, nb, nt, stats_cells(e)).total, e->st));
    v.forecast = M, v.nt = nt, v.blocks = nb;
    return CSIM_OK;
}

int csim_ensemble_verify_wait(csim_ensemble* e, const double** out_crps, const double** out_brier,
                              const unsigned long long** rank_hist, csim_verify_scores* scores) {
    CSIM_REQUIRE(e, "null ensemble");
    csim_ensemble::Verify& v = e->verify;
    CSIM_TRY(v.cap.wait("no verification in flight: csim_ensemble_verify_begin first"));
    const VerifyLayout l = verify_layout(v.forecast, v.blocks, v.nt, stats_cells(e));
    const double* const h = v.cap.host.as();
    if (out_crps) *out_crps = h + l.crps;
    if (out_brier) *out_brier = h + l.brier;
    if (rank_hist) *rank_hist = reinterpret_cast<const unsigned long long*>(h + l.hist);
    if (scores) verify_finish(reinterpret_cast<const unsigned long long*>(h + l.counts), h + l.sums, v.blocks, v.nt, scores);
    return CSIM_OK;
}

int csim_ensemble_rank_slot(long long g, int ties, int* slot) {
    CSIM_REQUIRE(slot && g >= 0 && ties >= 0, "bad argument");
    *slot = static_cast<int>(verify_mix(static_cast<unsigned long long>(g)) % (static_cast<unsigned long long>(ties) + 1));
    return CSIM_OK;
}

}  // extern "C"
