// ensemble_da.cpp — the ensemble's data assimilation: the EnSRF analysis of a plan, the seeded perturbations and the
// RTPS / RTPP relaxation (kernels in ensemble_assim.hip, ensemble_perturb.hip, ensemble_relax.hip; random numbers in
// ensemble_noise.hpp).  The plan, the Gaspari-Cohn table and the perturbation taps are made in assim_plan.cpp.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ensemble_host.hpp"
#include "ensemble_noise.hpp"

using namespace csim;

namespace {

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

int csim_ensemble_assimilate(csim_ensemble* e, int nobs, const int* i, const int* j, const double* y, const double* r,
                             double loc, double inflation, int truth_member, int ordered, double* prior_mean,
                             double* prior_var, double* post_mean, double* post_var, int* nlevels) {
    CSIM_REQUIRE(e, "null ensemble");
    const EnsGeom& g = e->g;
    CSIM_REQUIRE(nobs >= 0, "nobs must be >= 0");
    CSIM_REQUIRE(nobs == 0 || (i && j && y && r), "null observation array");
    CSIM_REQUIRE(std::isfinite(loc) && loc > 0, "loc must be finite and > 0");
    CSIM_REQUIRE(std::isfinite(inflation) && inflation >= 1.0, "inflation must be finite and >= 1");
    int M = 0, t = 0;
    CSIM_TRY(forecast_split(g.members, truth_member, &M, &t));
    CSIM_REQUIRE(ordered == 0 || ordered == 1, "ordered must be 0 or 1");
    CSIM_REQUIRE(M >= 2, "the analysis needs at least two forecast members");
    if (M > ASSIM_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate: at most 1024 forecast members");
    if (nobs > ASSIM_MAX_OBS) return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_assimilate: at most 2^20 observations");
    AssimPlan p;
    CSIM_TRY(assim_plan_build(g.nx, g.ny, e->dx, e->dy, loc, ordered == 1, nobs, i, j, r, y, &p));
    if (nlevels) *nlevels = p.nlevels;
    const bool diag = prior_mean || prior_var || post_mean || post_var;
    if (nobs == 0 && inflation == 1.0) return diag ? csim_ensemble_sync(e) : CSIM_OK;

    const size_t tcells = static_cast<size_t>(2 * p.lx + 1) * (2 * p.ly + 1);
    const int batch = assim_batch_size(M);
    const size_t hp = static_cast<size_t>(std::min(nobs, batch)) * M;
    const AssimLayout l = assim_layout(nobs, tcells, hp);

    // resources: the device buffer grows after the work already enqueued is done with it, the staging buffer after
    // its last copy has run
    void* h = nullptr;
    CSIM_TRY(e->assim.dev.reserve(l.total, e->st));
    CSIM_TRY(e->assim.stage.acquire(l.staged, &h));
    void* const d = e->assim.dev.p;
    double *hy = buf_at<double>(h, l.y), *hr = buf_at<double>(h, l.r);
    for (int q = 0; q < nobs; ++q) hy[q] = y[p.idx[q]], hr[q] = r[p.idx[q]];
    std::copy(p.pi.begin(), p.pi.end(), buf_at<int>(h, l.i));
    std::copy(p.pj.begin(), p.pj.end(), buf_at<int>(h, l.j));
    std::copy(p.idx.begin(), p.idx.end(), buf_at<int>(h, l.idx));
    gc_fill(e->dx, e->dy, loc, p.lx, p.ly, buf_at<double>(h, l.rho));
    CSIM_TRY(e->assim.stage.send(d, l.staged, e->st));

    const AssimObs obs{buf_at<int>(d, l.i), buf_at<int>(d, l.j), buf_at<int>(d, l.idx), buf_at<double>(d, l.y),
                       buf_at<double>(d, l.r)};
    const AssimArgs a = assim_args(M, t, p, buf_at<double>(d, l.rho), obs, buf_at<double>(d, l.scal),
                                   buf_at<double>(d, l.hp), prior_mean || prior_var ? buf_at<double>(d, l.prior) : nullptr);
    std::vector<AssimBatch> batches;
    assim_batches(g.nx, g.ny, p, batch, &batches);
    CSIM_TRY(assim_enqueue(e, a, inflation, batches));
    if (!diag) return CSIM_OK;
    double* post = buf_at<double>(d, l.post);
    if (post_mean || post_var) CSIM_HIP(ens_launch_assim_post(g, e->base(e->cur), a, nobs, post, e->st));
    // both copies are enqueued, then the call waits once
    std::vector<double> pr(2 * static_cast<size_t>(nobs)), po(2 * static_cast<size_t>(nobs));
    if (a.prior && nobs)
        CSIM_HIP(hipMemcpyAsync(pr.data(), a.prior, sizeof(double) * pr.size(), hipMemcpyDeviceToHost, e->st));
    if ((post_mean || post_var) && nobs)
        CSIM_HIP(hipMemcpyAsync(po.data(), post, sizeof(double) * po.size(), hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    split_pairs(pr.data(), nobs, prior_mean, prior_var);
    split_pairs(po.data(), nobs, post_mean, post_var);
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
    CSIM_HIP(ens_launch_perturb(g, e->base(e->cur), a, centered == 1, e->st, e->perturb.tile_rows,
                                e->perturb.member_shares));
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
