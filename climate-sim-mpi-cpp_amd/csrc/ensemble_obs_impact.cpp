// ensemble_obs_impact.cpp — the forecast impact of a network's observations (csim_obs_network_impact_capture,
// csim_ensemble_obs_impact and _impact_global of include/csim.h; kernels in ensemble_impact.hip and ensemble_dot.hip;
// the network is obs_network.hpp's).  A capture lives in storage of the network's own, made at the first capture: a_k
// per observation, dn and the status bytes, and a device copy of the caller's weight; nothing that an analysis,
// observe or set_values writes.
// csim_ensemble_obs_impact_global reads the same capture without the localisation: the weight goes through the
// ensemble-space dot (dot_stage_fields, dot_enqueue of ensemble_space.cpp), then one kernel of ensemble_dot.hip.  The
// two calls differ in that, the staging of the weight and the launch; their checks and what they bring back are one
// text (impact_check, impact_run).
#include <new>
#include <string>
#include <vector>

#include "obs_network.hpp"

using namespace csim;

namespace {

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
    if (n->hold.last)
        return fail(CSIM_ERR_STATE, "csim_obs_network_impact_capture: the network's last analysis was a held one "
                                    "(csim_ensemble_assimilate_etkf_held); the forecast impact of held observations is "
                                    "not built");
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

}  // extern "C"
