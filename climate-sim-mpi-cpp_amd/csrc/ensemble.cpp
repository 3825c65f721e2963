// ensemble.cpp — csim_ensemble_*: B single-rank members of one grid shape on one GPU, stepped together (kernels in
// ensemble.hip, device layout in ensemble.hpp).  Each member is advanced exactly as csim_stepper_run advances a
// single-rank stepper holding the same field with the same parameters, ghost ring included.
// Layout of the ensemble's host side, behind ensemble_host.hpp (the handle and the helpers its features share):
//   ensemble.cpp       the handle: create / destroy, upload / download / init_gaussian, physics and the member table,
//                      the pass plan and sign classes, run / sync, per-member reductions, options
//   ensemble_diag.cpp  diagnostics, synchronous and as _begin / _wait captures: statistics, quantiles (and their
//                      plan), verification (and its rank slot)
//   ensemble_spatial.cpp  neighbourhood and probability verification (tables, window sums), its overflow bound and the
//                      host-only finishing of the tables into scores
//   ensemble_da.cpp    data assimilation: the analysis of a plan, Philox / normal numbers, perturbations, relaxation
//                      (prior capture, relax); the plan, the Gaspari-Cohn table and the taps: assim_plan.cpp, without HIP
//   ensemble_obs.cpp   observation networks (obs_network.hpp): create / destroy, values from the host or from a member,
//                      the mask, fetch, the logs and the status bytes
//   ensemble_analysis.cpp  the analyses that read a network: the serial one with its diagnostics and log, the local
//                      analysis, the ETKF and the LETKF (the LETKF's lattice and node storage: letkf_nodes.hpp, its
//                      lookup: assim_plan.cpp, without HIP)
//   ensemble_obs_impact.cpp  the forecast impact of a network's observations: capture, local and global impact
//   ensemble_space.cpp ensemble space: Gram matrix, projection, transform, dot and EOFs; the eigensolver:
//                      sym_eigen.cpp, without HIP
#include <cmath>
#include <string>
#include <vector>

#include "ensemble_host.hpp"
#include "sym_eigen.hpp"

using namespace csim;

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
        cls[m] = sign_class(p);
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

// the stream and the device memory of a new ensemble
int make_resources(csim_ensemble* e, size_t bytes, size_t nred) {
    const int B = e->g.members;
    CSIM_TRY(e->own.stream(&e->st));
    // zero-filled: the pads and the device-only ghost layers the multi-step sweep reads as don't-care must be finite
    CSIM_TRY(e->own.device(&e->alloc[0], bytes, true));
    CSIM_TRY(e->own.device(&e->alloc[1], bytes, true));
    CSIM_TRY(e->own.device(&e->fin, sizeof(double) * e->g.fin_stride * B, true));
    CSIM_TRY(e->own.device(&e->table, ens_entry_bytes() * B));
    CSIM_TRY(e->own.device(&e->order, sizeof(int) * B));
    return e->own.device(&e->scratch, sizeof(double) * nred);
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
    *cls = sign_class(p);
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
    if (make_resources(e, bytes, nred) != CSIM_OK) {
        const std::string why = csim_last_error();
        csim_ensemble_destroy(e);
        return fail(CSIM_ERR_HIP, "csim_ensemble_create: " + why);
    }
    *out = e;
    return CSIM_OK;
}

int csim_ensemble_destroy(csim_ensemble* e) {
    if (!e) return CSIM_OK;
    e->own.drain();
    e->obs.release();
    e->stats.release();
    e->quant.release();
    e->verify.release();
    e->spatial.release();
    e->assim.release();
    e->relax.release();
    e->espace.release();
    e->letkf.release();
    e->own.release();
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
        CSIM_TRY(csim_ensemble_upload(e, m, host + per * m));
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
        CSIM_TRY(csim_ensemble_download(e, m, host + per * m));
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
    CSIM_TRY(csim_ensemble_plan(nsteps, e->g.nx, e->g.ny, e->fuse, plan));
    CSIM_TRY(ensure_tables(e));
    const int q = plan[1], r = plan[2];
    const bool stat = e->static_ring();
    if (nsteps > 0) e->relax.mode = 0;  // the forecast a relaxation capture was taken of is gone
    // q passes of ENS_DEPTH steps, one launch per sign class present; the last one of the run leaves the FinLines
    // (unless the ring is static) from which the closing ghost fill makes the reference's ring
    for (int k = 0; k < q; ++k) {
        if (!e->ring_ok) {
            CSIM_TRY(ghost_fill(e, false));
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
            CSIM_TRY(ghost_fill(e, true));
        }
    }
    for (int k = 0; k < r; ++k) {
        if (!e->ring_ok) {
            CSIM_TRY(ghost_fill(e, false));
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

// the ensemble's members for the reductions of internal.hpp
static Members members_of(const csim_ensemble* e) { return {e->g.members, e->g.slab, ENS_REDUCE_ROWS}; }

int csim_ensemble_checksum(csim_ensemble* e, unsigned long long* out) {
    CSIM_REQUIRE(e && out, "null argument");
    const Members mb = members_of(e);
    CSIM_HIP(launch_checksum(e->base(e->cur), e->g.nx, e->g.ny, e->g.pitch, 0, 0, e->g.nx, e->scratch, e->st, mb));
    return fold_checksum(e->scratch, e->g.ny, out, e->st, mb);
}

int csim_ensemble_minmax(csim_ensemble* e, double* out) {
    CSIM_REQUIRE(e && out, "null argument");
    const Members mb = members_of(e);
    CSIM_HIP(launch_minmax(e->base(e->cur), e->g.nx, e->g.ny, e->g.pitch, e->scratch, e->st, mb));
    return fold_partials(e->scratch, e->g.ny + 2, 0, out, e->st, mb);
}

int csim_ensemble_sum(csim_ensemble* e, double* out) {
    CSIM_REQUIRE(e && out, "null argument");
    const Members mb = members_of(e);
    CSIM_HIP(launch_sum(e->base(e->cur), e->g.nx, e->g.ny, e->g.pitch, e->scratch, e->st, mb));
    return fold_partials(e->scratch, e->g.ny, 1, out, e->st, mb);
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
    } else if (k == "spatial_grid_max") {
        CSIM_REQUIRE(value >= 0 && value <= 65535, "spatial_grid_max must be 0 (automatic) or 1 .. 65535");
        e->spatial.grid_max = static_cast<int>(value);
    } else if (k == "spatial_member_split") {
        CSIM_REQUIRE(value >= 0 && value <= 4096, "spatial_member_split must be 0 (automatic) or 1 .. 4096");
        e->spatial.member_split = static_cast<int>(value);
    } else if (k == "perturb_tile_rows") {
        CSIM_REQUIRE(value == 0 || value == 8 || value == 32, "perturb_tile_rows must be 0 (automatic), 8 or 32");
        e->perturb.tile_rows = static_cast<int>(value);
    } else if (k == "perturb_member_shares") {
        CSIM_REQUIRE(value >= 0 && value <= 65535, "perturb_member_shares must be 0 (automatic) or 1 .. 65535");
        e->perturb.member_shares = static_cast<int>(value);
    } else if (k == "local_tile") {
        CSIM_REQUIRE(value == 0 || value == 4 || value == 8 || value == 16, "local_tile must be 0 (automatic), 4, 8 or 16");
        e->local.tile = static_cast<int>(value);
    } else if (k == "local_pack") {
        CSIM_REQUIRE(value >= 0 && value <= 64, "local_pack must be 0 (automatic) or 1 .. 64");
        e->local.pack = static_cast<int>(value);
    } else if (k == "gram_form") {
        CSIM_REQUIRE(value >= 0 && value <= GRAM_FORMS, "gram_form must be 0 (automatic) or 1 .. 3");
        e->espace.gram_form = static_cast<int>(value);
    } else if (k == "project_form") {
        CSIM_REQUIRE(value >= 0 && value <= PROJECT_FORMS, "project_form must be 0 (automatic) or 1");
        e->espace.project_form = static_cast<int>(value);
    } else if (k == "obs_gram_form") {
        CSIM_REQUIRE(value >= 0 && value <= GRAM_FORMS, "obs_gram_form must be 0 (automatic) or 1 .. 3");
        e->espace.obs_gram_form = static_cast<int>(value);
    } else if (k == "eigen_form") {
        CSIM_REQUIRE(value >= 0 && value <= EIGEN_FORMS, "eigen_form must be 0 (automatic) or 1 .. 3");
        e->espace.eigen_form = static_cast<int>(value);
    } else if (k == "letkf_form") {
        CSIM_REQUIRE(value >= 0 && value <= LETKF_FORMS, "letkf_form must be 0 (automatic) or 1");
        e->letkf.form = static_cast<int>(value);
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
    else if (k == "spatial_grid_max")
        *value = e->spatial.grid_max;
    else if (k == "spatial_member_split")
        *value = e->spatial.member_split;
    else if (k == "perturb_tile_rows")
        *value = e->perturb.tile_rows;
    else if (k == "perturb_member_shares")
        *value = e->perturb.member_shares;
    else if (k == "local_tile")
        *value = e->local.tile;
    else if (k == "local_pack")
        *value = e->local.pack;
    else if (k == "gram_form")
        *value = e->espace.gram_form;
    else if (k == "project_form")
        *value = e->espace.project_form;
    else if (k == "obs_gram_form")
        *value = e->espace.obs_gram_form;
    else if (k == "eigen_form")
        *value = e->espace.eigen_form;
    else if (k == "letkf_form")
        *value = e->letkf.form;
    else if (k == "contract")
        return fail(CSIM_ERR_UNSUPPORTED, "an ensemble is always bit-identical: no contract mode");
    else
        return fail(CSIM_ERR_ARG, "unknown option " + k);
    return CSIM_OK;
}

}  // extern "C"
