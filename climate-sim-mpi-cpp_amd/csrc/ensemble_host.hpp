// ensemble_host.hpp — what the host translation units behind csim_ensemble_* share: the ensemble handle and the helpers
// of the analysis.  The small owning types its features are built from are owned.hpp's (through stepper.hpp).  Host
// only: the device translation units compile ensemble.hpp and never see this file.  The layout of the ensemble's host
// side is the table at the top of ensemble.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "assim_plan.hpp"
#include "ensemble.hpp"
#include "letkf_nodes.hpp"
#include "stepper.hpp"

namespace csim {

// Of B members, *M are forecast members and member *t is the truth that is left out (*t = B: none): forecast member k
// is member k + (k >= *t).  With min_msg, *M >= min_m is required; with max_msg, more than max_m are unsupported.
// The verification and the analysis pass neither and make those two checks themselves, because they have other
// argument checks that fire between the range check and the bounds, and the order in which checks fire is kept.
inline int forecast_split(int B, int truth_member, int* M, int* t, int min_m = 0, const char* min_msg = nullptr,
                          int max_m = 0, const char* max_msg = nullptr) {
    CSIM_REQUIRE(truth_member >= -1 && truth_member < B, "truth_member out of range");
    *M = truth_member >= 0 ? B - 1 : B;
    *t = truth_member >= 0 ? truth_member : B;
    if (min_msg) CSIM_REQUIRE(*M >= min_m, min_msg);
    if (max_msg && *M > max_m) return fail(CSIM_ERR_UNSUPPORTED, max_msg);
    return CSIM_OK;
}

}  // namespace csim

struct csim_ensemble {
    csim::EnsGeom g{};
    double dx = 1.0, dy = 1.0;
    csim::Owned own;                  // what csim_ensemble_create made; the six pointers and the stream below are views
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
    int class_off[csim::ENS_CLASSES + 1] = {};
    bool ring_ok = false;             // ghost rings filled and static (no Neumann side)
    int fuse = -1, fused_2c = 1, depth_used = 0;

    // What each feature owns, created on its first use and given back by its release().
    // per-cell statistics (csim_ensemble_stats*): mean, var, min, max
    struct Stats {
        csim::Capture cap;
        void release() { cap.release(); }
    } stats;
    // per-cell quantiles (csim_ensemble_quantiles*): nq quantile fields, then the exceedance fields
    struct Quant {
        csim::Capture cap;
        int nq = 0;  // levels of the capture in flight
        void release() { cap.release(); }
    } quant;
    // verification (csim_ensemble_verify*): one buffer (VerifyLayout), and the device copy of a host truth
    struct Verify {
        csim::Capture cap;
        csim::DeviceBuf truth;
        csim::Staging stage;
        int forecast = 0, nt = 0, blocks = 0;  // of the capture in flight
        void release() { cap.release(), truth.release(), stage.release(); }
    } verify;
    // neighbourhood and probability verification (csim_ensemble_verify_spatial*, ensemble_spatial.cpp): one buffer
    // (SpatialLayout), the device copy of a host truth, and its two options
    struct Spatial {
        csim::Capture cap;
        csim::DeviceBuf truth;
        csim::Staging stage;
        int forecast = 0, nt = 0, ns = 0, fields = 0;  // of the capture in flight
        int grid_max = 0, member_split = 0;            // options spatial_grid_max, spatial_member_split; 0: automatic
        void release() { cap.release(), truth.release(), stage.release(); }
    } spatial;
    // analysis (csim_ensemble_assimilate): one device buffer (AssimLayout) and the staging of its inputs
    struct Assim {
        csim::DeviceBuf dev;
        csim::Staging stage;
        void release() { dev.release(), stage.release(); }
    } assim;
    // perturbations (csim_ensemble_perturb): no storage, its two launch options
    struct Perturb {
        int tile_rows = 0, member_shares = 0;  // options perturb_tile_rows, perturb_member_shares; 0: automatic
    } perturb;
    // the local analysis (csim_ensemble_assimilate_local): no storage of the ensemble's, its two launch options
    struct Local {
        int tile = 0, pack = 0;  // options local_tile, local_pack; 0: automatic
    } local;
    // relaxation (csim_ensemble_prior_capture / csim_ensemble_relax).  A capture lives in the handle's own storage, so
    // that no call that writes the ping-pong buffers touches it: sqrt(v_b) per interior cell (RTPS), a copy of the
    // current buffer (RTPP, allocated at the first such capture), and the factor field of a call that asks for it
    struct Relax {
        csim::DeviceBuf sb, prior, factor;
        int mode = 0;    // mode of the valid capture; 0: none (cleared by a run of nsteps > 0)
        int truth = -1;  // its truth_member
        void release() { sb.release(), prior.release(), factor.release(); }
    } relax;
    // ensemble space (csim_ensemble_gram, _project, _transform, _eofs; ensemble_space.cpp): the class partials and G
    // of the Gram matrix, the output fields of a projection, W (and wbar) on the device with their staging, and its
    // two launch options
    struct Espace {
        csim::DeviceBuf partial, gram, out, w;
        csim::Staging stage;
        int gram_form = 0, project_form = 0;  // options gram_form, project_form; 0: automatic
        // the observation-space Gram matrix (csim_ensemble_obs_gram, ensemble_analysis.cpp) shares `partial` and `gram`;
        // what the last completed csim_ensemble_assimilate_etkf found, for csim_ensemble_etkf_info
        int obs_gram_form = 0;                // option obs_gram_form; 0: automatic
        bool etkf_valid = false;
        long long etkf_used = 0;
        double etkf_chi2 = 0.0, etkf_dfs = 0.0;
        std::vector<double> etkf_gamma;
        // the device ETKF (csim_ensemble_assimilate_etkf_device): the solver's working matrices, V, lambda and info, and
        // the record with gamma behind it (EtkfLayout); csim_ensemble_etkf_info fetches a pending record
        csim::DeviceBuf eig;
        int eigen_form = 0;                   // option eigen_form; 0: by the number of members
        bool etkf_pending = false;            // the last ETKF was enqueued by the device path: its record is on the device
        int etkf_m = 0;                       // its forecast members
        int etkf_sweeps = 0, etkf_status = 0; // of the record fetched last (0 after a host-path ETKF)
        // csim_ensemble_dot (and the g of csim_ensemble_obs_impact_global): the fields' interiors, the class partials
        // and the M x K result; a host call stages its fields through `stage`
        csim::DeviceBuf dot_fields, dot_partial, dot_out;
        void release() {
            partial.release(), gram.release(), out.release(), w.release(), eig.release(), stage.release();
            dot_fields.release(), dot_partial.release(), dot_out.release();
        }
    } espace;
    // the LETKF (csim_ensemble_assimilate_letkf, ensemble_analysis.cpp): the node storage of the last call (LetkfLayout) and
    // what csim_ensemble_letkf_info needs to fetch its record; its launch option
    struct Letkf {
        csim::DeviceBuf buf;
        csim::LetkfLayout l{};
        int form = 0;            // option letkf_form; 0: automatic
        bool valid = false;      // there was an LETKF, and `buf` still holds its record
        int nax = 0, nay = 0;    // its lattice
        void release() { buf.release(); }
    } letkf;
    // observation networks (csim_obs_network_*, ensemble_obs.cpp; the type: obs_network.hpp): the ones that are alive; each owns its device buffer
    struct Obs {
        std::vector<csim_obs_network*> nets;
        void release();  // destroys them
    } obs;

    double* view(int buf, int m) const {
        return alloc[buf] + static_cast<size_t>(m) * g.slab + static_cast<size_t>(csim::GHOST_EXTRA) * g.pitch;
    }
    double* base(int buf) const { return alloc[buf] + static_cast<size_t>(csim::GHOST_EXTRA) * g.pitch; }
    bool static_ring() const {
        for (int k = 0; k < 4; ++k)
            if (g.bc[k] == CSIM_BC_NEUMANN) return false;
        return true;
    }
};

namespace csim {
// the doubles of Espace::eig for M forecast members
struct EtkfLayout {
    size_t work, V, lam, rec, gamma, info, doubles;
    explicit EtkfLayout(int M) {
        const size_t m = static_cast<size_t>(M);
        static_assert(sizeof(EtkfRecord) == 4 * sizeof(double), "the record is four doubles, gamma follows it");
        work = 0, V = 2 * m * m, lam = V + m * m, rec = lam + m, gamma = rec + 4, info = gamma + m, doubles = info + 1;
    }
};
// cells of a dense per-cell field, ghost ring included
inline size_t stats_cells(const csim_ensemble* e) { return static_cast<size_t>(e->g.nx + 2) * (e->g.ny + 2); }

// The launches of an analysis (ensemble_da.cpp) of a plan (assim_plan.hpp), shared by csim_ensemble_assimilate and
// csim_ensemble_assimilate_network.  h'_k of one batch: 64 MiB, at least 8192 observations
constexpr size_t ASSIM_HP_DOUBLES = size_t(1) << 23;
inline int assim_batch_size(int M) { return static_cast<int>(std::min<size_t>(ASSIM_HP_DOUBLES / M, ASSIM_MAX_OBS)); }
// the arguments of the analysis kernels for M forecast members without member t, from the device arrays of a plan's
// observations; a linear network adds its taps, a screened analysis sets `status` afterwards
inline AssimArgs assim_args(int M, int t, const AssimPlan& p, const double* rho, const AssimObs& obs, double* scal,
                            double* hp, double* prior, const int* tstart = nullptr, const int* toff = nullptr,
                            const double* tw = nullptr, int tmax = 0) {
    AssimArgs a{};
    a.forecast = M, a.truth_member = t, a.lx = p.lx, a.ly = p.ly;
    a.rho = rho, a.obs = obs;
    a.scal = scal, a.hp = hp, a.prior = prior;
    a.tstart = tstart, a.toff = toff, a.tw = tw, a.tmax = tmax;  // null / 0: point observations
    return a;
}
// n (mean, variance) pairs by input index, already on the host -> two arrays, either may be null
inline void split_pairs(const double* pairs, int n, double* mean, double* var) {
    for (int o = 0; mean && o < n; ++o) mean[o] = pairs[2 * static_cast<size_t>(o)];
    for (int o = 0; var && o < n; ++o) var[o] = pairs[2 * static_cast<size_t>(o) + 1];
}
// the inflation (when != 1), then assim_prior and assim_update of every batch in turn, on the ensemble's stream
int assim_enqueue(csim_ensemble* e, const AssimArgs& a, double inflation, const std::vector<AssimBatch>& batches);
// csim_ensemble_dot in two steps (ensemble_space.cpp), shared with csim_ensemble_obs_impact_global: the interiors of K
// host fields of the layout (ny+2) x (nx+2) to espace.dot_fields, copied before the call returns; then the two
// launches for M forecast members without member t, which leave the M x K result in espace.dot_out
int dot_stage_fields(csim_ensemble* e, int K, const double* fields);
// every interior value of a host field of the layout (ny+2) x (nx+2) is finite: no exponent field is all ones.  A row
// at a time without a branch per value, so that the check of a large field costs a pass over it and no more
inline bool interior_finite(const double* field, int nx, int ny) {
    std::uint64_t bad = 0;
    for (int j = 1; j <= ny; ++j) {
        const double* row = field + static_cast<size_t>(j) * (static_cast<size_t>(nx) + 2) + 1;
        for (int i = 0; i < nx; ++i) {
            std::uint64_t b;
            std::memcpy(&b, row + i, sizeof b);
            bad |= static_cast<std::uint64_t>(((b >> 52) & 0x7ff) == 0x7ff);
        }
    }
    return bad == 0;
}
int dot_enqueue(csim_ensemble* e, int M, int t, bool centered, int K);
}  // namespace csim
