// ensemble.hpp — the batched engine behind csim_ensemble_* (include/csim.h): B members of one grid shape, each with
// its own field and its own (D, dt, vx, vy), stepped together, every kernel launch covering all members (or all
// members of one upwind-sign class).
//
// Device layout: two allocations (ping / pong), each B member slabs of csim_field's padded layout one after the
// other, slab = (ny + 2 + 2 GHOST_EXTRA) * pitch doubles, so every member starts 128-byte aligned like a csim_field.
// Member m's row j = 0 is at  alloc + m * slab + GHOST_EXTRA * pitch.
#pragma once

#include "gram_plan.hpp"
#include "internal.hpp"

namespace csim {

// The one depth the batched multi-step sweep is instantiated at (profiles/r04_ensemble_depth.jsonl: full ensembles of
// 256^2 and 512^2 members, T = 4 against T = 6).  -DCSIM_ENS_T=6 builds the other one for that measurement.
#ifndef CSIM_ENS_T
#define CSIM_ENS_T 4
#endif
constexpr int ENS_DEPTH = CSIM_ENS_T;
static_assert(ENS_DEPTH >= 2 && ENS_DEPTH <= MAX_FUSE, "ensemble depth out of range");

// upwind-sign flavours of a member (the launch it belongs to): the values of sign_class (internal.hpp), which is also
// how the single stepper's launcher picks k_sweepO_dpp<., ., SX, SY>
constexpr int ENS_CLASSES = 9;

struct EnsGeom {
    int members;
    int nx, ny, pitch;
    long slab;    // doubles from one member's slab to the next
    long fin_stride;  // doubles of FinLines per member: left, right (ly each), bottom, top (lx each), all 16-B aligned
    int ly, lx;   // ny, nx rounded up to even
    int div_mode;
    int bc[4];
    double value;
};

// per-member device table: one opaque entry per member (Phys + FinLines pointers)
size_t ens_entry_bytes();
void ens_entry_fill(void* host_entry, const Phys& p, double* const fin_lines[4]);

// T = ENS_DEPTH steps of the members members[0 .. count) (all of one sign class `cls`) in one launch;
// fin: last pass of a run, the members' FinLines are written (see FinLines in sweep_core.hpp)
hipError_t ens_launch_sweepO(const EnsGeom& g, const double* in, double* out, const void* table, const int* members,
                             int count, int cls, bool fin, hipStream_t st);
// one step of every member
hipError_t ens_launch_step(const EnsGeom& g, const double* in, double* out, const void* table, hipStream_t st);
// apply_boundary of every member into a and b; fin: Neumann ghosts from the members' FinLines
hipError_t ens_launch_ghost_fill(const EnsGeom& g, double* a, double* b, const void* table, bool fin, hipStream_t st);
// per-member reductions: the launchers and folds of internal.hpp with this cap (scratch: members * 2 * 64 doubles)
constexpr int ENS_REDUCE_ROWS = 64;

// per-cell statistics over all members (ensemble_stats.hip), one launch: out = mean, var (divided by members - ddof),
// min, max, each dense (ny+2) x (nx+2); members beyond STATS_LDS_MEMBERS are read twice
constexpr int STATS_LDS_MEMBERS = 320;  // 320 x 64 cells x 8 B = 160 KiB of LDS
hipError_t ens_launch_stats(const EnsGeom& g, const double* f, int ddof, double* out, hipStream_t st);

// per-cell quantiles and exceedance probabilities over all members (ensemble_quantiles.hip), one launch: out = nq
// quantile fields, then nt exceedance fields, each dense (ny+2) x (nx+2).  (lo[k], hi[k], g[k]): numpy's "linear" plan
// of level k for this many members (csim_ensemble_quantile_plan)
constexpr int QUANT_MAX_LEVELS = 16;       // levels and thresholds per call, each
constexpr int QUANT_MAX_MEMBERS = 4096;    // the largest sorting network instantiated (64 values per lane of a wave)
struct QuantArgs {
    int nq, nt;
    int lo[QUANT_MAX_LEVELS], hi[QUANT_MAX_LEVELS];
    double g[QUANT_MAX_LEVELS];
    double thr[QUANT_MAX_LEVELS];
};
hipError_t ens_launch_quantiles(const EnsGeom& g, const double* f, const QuantArgs& qa, double* out, hipStream_t st);

// ensemble verification against one truth per cell (ensemble_verify.hip), one launch: the per-cell CRPS and Brier
// scores (dense (ny+2) x (nx+2) each), the rank histogram of the interior (M + 1 bins, one integer atomic per bin and
// workgroup into `hist`, which the caller zeroes), and per-workgroup partial sums of the domain scores, which the host
// adds in workgroup order.  M forecast members: all B with a truth field, or the B - 1 others with truth member t.
constexpr int VERIFY_MAX_THRESHOLDS = 16;
constexpr int VERIFY_MAX_MEMBERS = QUANT_MAX_MEMBERS;  // forecast members, the largest sorting network
constexpr int VERIFY_SUMS = 3 + VERIFY_MAX_THRESHOLDS;  // partials per workgroup: CRPS, (m - y)^2, var, Brier[16]
constexpr int VERIFY_GRID_MAX = 1024;                   // workgroups per launch, at most (each loops over its tiles)
struct VerifyArgs {
    int forecast;          // M
    int truth_member;      // t, or B with `truth` (then no member is skipped)
    int nt;
    int fair;
    const double* truth;   // device, dense (ny+2) x (nx+2); null with a truth member
    double thr[VERIFY_MAX_THRESHOLDS];
};
struct VerifyOut {
    double* crps;               // one field
    double* brier;              // nt fields
    unsigned long long* hist;   // M + 1 bins, zeroed by the caller
    unsigned long long* counts; // per workgroup: non-NaN interior cells, NaN interior cells
    double* sums;               // per workgroup: VERIFY_SUMS partial sums over the non-NaN interior cells
};
int ens_verify_blocks(const EnsGeom& g, int forecast);  // workgroups of the launch: records in counts / sums
hipError_t ens_launch_verify(const EnsGeom& g, const double* f, const VerifyArgs& va, const VerifyOut& o,
                             hipStream_t st);

// neighbourhood and probability verification (ensemble_spatial.hip, csim_ensemble_verify_spatial): integers only.
// Pass 1, ens_launch_spatial_counts: one read of the members -> the count planes n_q (uint16, nt planes of ny x nx, no
// ghost ring) and the flags word per interior cell (bit q = o_q, bit 31 = NaN cell).  With split > 1 the members of a
// cell are divided over blockIdx.y, the parts add into `acc` (32-bit atomics; nt + 1 planes, the last one the NaN
// marks, zeroed by the launcher) and a merge kernel writes counts and flags.
// Pass 2, ens_launch_spatial_scores: reads only counts and flags; per threshold the contingency table and, per scale,
// the sums A, Bo, C over square windows, from a summed-area table in LDS.  Both loop under a cap on gridDim.x.
constexpr int SPATIAL_MAX_HALF = 32;
constexpr int SPATIAL_MAX_SCALES = 8;
constexpr int SPATIAL_TILE = 32;               // centres per tile side of pass 2
constexpr int SPATIAL_COUNTS_GRID_MAX = 2048;  // default caps on gridDim.x
constexpr int SPATIAL_SCORES_GRID_MAX = 1024;
struct SpatialArgs {
    int forecast;          // M
    int truth_member;      // t, or B with `truth`
    int nt, ns;
    int hmax;              // the call's largest half-width (0 without scales)
    int split;             // parts of the members in pass 1, >= 1
    int grid_max;          // cap on gridDim.x of both passes; 0: the defaults above
    const double* truth;   // device, dense (ny+2) x (nx+2); null with a truth member
    int half[SPATIAL_MAX_SCALES];
    double thr[VERIFY_MAX_THRESHOLDS];
};
struct SpatialOut {
    unsigned long long* table;   // nt x (M + 1) x 2, zeroed by the caller
    unsigned long long* nbh;     // nt x ns x 3, zeroed by the caller
    unsigned long long* cells;   // 2: non-NaN and NaN interior cells, zeroed by the caller
    unsigned* flags;             // nx ny
    unsigned short* counts;      // nt x nx ny
    unsigned* acc;               // (nt + 1) x nx ny, used with split > 1
};
int ens_spatial_split(int cells, int forecast);  // the default split of pass 1
size_t ens_spatial_lds(int forecast, int hmax);  // dynamic LDS of a workgroup of pass 2, bytes
hipError_t ens_launch_spatial_counts(const EnsGeom& g, const double* f, const SpatialArgs& a, const SpatialOut& o,
                                     hipStream_t st);
hipError_t ens_launch_spatial_scores(const EnsGeom& g, const SpatialArgs& a, const SpatialOut& o, hipStream_t st);

// the analysis (ensemble_assim.hip): the serial EnSRF of csim.h, one level of mutually non-conflicting observations
// after the other, two launches per batch of a level: assim_prior (one wave per observation: h'_k and its scalars)
// and assim_update (one wave per 64 cells of one observation's window).  Observations are in plan order; `first` is
// the batch's first plan position, `count` its observations.
constexpr int ASSIM_MAX_MEMBERS = 1024;
constexpr int ASSIM_MAX_OBS = 1 << 20;
struct AssimObs {                 // device arrays, plan order
    const int* i;
    const int* j;
    const int* idx;               // input index (the diagnostics are in input order)
    const double* y;
    const double* r;
};
struct AssimArgs {
    int forecast;                 // M
    int truth_member;             // t, or B (no member skipped)
    int lx, ly;
    const double* rho;            // (2 ly + 1) x (2 lx + 1)
    AssimObs obs;
    double* scal;                 // 3 per plan position: d, alpha, delta
    double* hp;                   // M per observation of the batch: h'_k
    double* prior;                // 2 per input index: hbar, p (null: not wanted)
    // linear observations (csim_obs_network_create_linear); null / 0: point observations.  Last, so that the
    // arguments of the point kernels stay where they were
    const int* tstart;            // plan order, one more than observations: the taps of position q are
                                  // tstart[q] .. tstart[q + 1] - 1
    const int* toff;              // per tap: dj * pitch + di, the cell's offset from the anchor in a member's slab
    const double* tw;             // per tap: w
    int tmax;                     // the most taps of one observation (sizes the linear prior's LDS tile)
    // screening (csim_ensemble_assimilate_screened): one byte per plan position, an observation whose byte is not 0
    // (CSIM_OBS_USED) takes no turn; null: every observation is used.  After the taps, for the same reason
    const unsigned char* status;
};
// the batch's h'_k and scalars, then its window updates; wcells: the largest clipped window of the batch in cells.
// With taps (a.tstart) the prior is the linear one: h_k = sum_s w_s x_k(anchor + tap s)
hipError_t ens_launch_assim_prior(const EnsGeom& g, const double* f, const AssimArgs& a, int first, int count,
                                  hipStream_t st);
hipError_t ens_launch_assim_update(const EnsGeom& g, double* f, const AssimArgs& a, int first, int count,
                                   long wcells, hipStream_t st);
// x_k <- x_k + lm1 (x_k - xbar) on every interior cell of the forecast members
hipError_t ens_launch_assim_inflate(const EnsGeom& g, double* f, int forecast, int truth_member, double lm1,
                                    hipStream_t st);
// the posterior mean and variance at each observation's cell (with taps: of its h_k), 2 per input index
hipError_t ens_launch_assim_post(const EnsGeom& g, const double* f, const AssimArgs& a, int nobs, double* post,
                                 hipStream_t st);

// the per-observation forecast impact (ensemble_impact.hip): csim_obs_network_impact_capture and
// csim_ensemble_obs_impact.  Everything is in plan order but `bg` and the result, which go by input index.
struct ImpactCapture {
    const double* bg;             // 2 per input index: hb, vb of the recorded analysis
    const unsigned char* status;  // that analysis's status bytes; null: it was not screened, every observation was used
    double* pert;                 // M per plan position: a_k = h_k - ha
    double* dn;                   // (y - hb) / r
    unsigned char* snap;          // the status bytes, kept
};
struct ImpactArgs {
    int nobs;
    int forecast;                 // M
    int truth_member;             // t, or B (no member skipped)
    int lx, ly;
    const double* rho;            // (2 ly + 1) x (2 lx + 1)
    const int* i;
    const int* j;
    const int* idx;
    const unsigned char* snap;
    const double* pert;
    const double* dn;
    const double* w;              // the weight, dense (ny+2) x (nx+2)
};
// a_k, dn and the status of every observation from the current members; the AssimArgs as for ens_launch_assim_post
hipError_t ens_launch_impact_capture(const EnsGeom& g, const double* f, const AssimArgs& a, int nobs,
                                     const ImpactCapture& c, hipStream_t st);
// J_o of every observation, by input index, from the members at verification time
hipError_t ens_launch_obs_impact(const EnsGeom& g, const double* f, const ImpactArgs& a, double* out, hipStream_t st);

// the local analysis of csim_ensemble_assimilate_local (ensemble_local.hip): the observation priors h_{o,k} of the used
// observations (one wave per observation, `prior`: M doubles per plan position), then the cell pass, one wave per
// `pack` cells of one tile of the host's lookup (LocalTiles of assim_plan.hpp, on the device).  The AssimArgs as for
// ens_launch_assim_post, with `status` where the analysis is screened.
constexpr int LOCAL_MAX_OBS = 64;        // CSIM_LOCAL_MAX_OBS
constexpr int LOCAL_MAX_DOUBLES = 4096;  // CSIM_LOCAL_MAX_DOUBLES
struct LocalArgs {
    int tile, ntx, nty;           // tiles of tile x tile cells, ntx x nty of them
    int lmax;                     // the network's max_local: a cell's lanes are lmax + 1
    int pack;                     // cells per wave, from ens_local_pack
    const int* cstart;            // per tile, one more than tiles: its entries are cpos[cstart[T]] .. cpos[cstart[T + 1] - 1]
    const int* cpos;              // plan positions, sorted by input index within a tile
    const double* prior;          // M per plan position: h_{o,k}
};
// cells per wave for M forecast members and max_local = lmax: `want` (0: as many as fit) cut to what the lanes of a
// wave and its LDS hold, at least 1
int ens_local_pack(int M, int lmax, int want);
hipError_t ens_launch_local_prior(const EnsGeom& g, const double* f, const AssimArgs& a, int nobs, double* prior,
                                  hipStream_t st);
hipError_t ens_launch_local_update(const EnsGeom& g, double* f, const AssimArgs& a, const LocalArgs& l, hipStream_t st);

// the perturbation of csim_ensemble_perturb (ensemble_perturb.hip), one launch: x_k += sigma p_k on every interior
// cell of the forecast members, p_k the white noise of ensemble_noise.hpp smoothed with the host's taps along x, then
// along y (csim_ensemble_perturb_taps; tx[o + rx], ty[o + ry]), less its mean over the members when centered
constexpr int PERTURB_TAPS = 2 * 32 + 1;  // 2 CSIM_PERTURB_MAX_RADIUS + 1
struct PerturbArgs {
    unsigned seed_lo, seed_hi, draw;
    int forecast;                 // M
    int truth_member;             // t, or B (no member skipped)
    int rx, ry;                   // tap radii
    int perx, pery;               // axis periodic
    double sigma;
    double tx[PERTURB_TAPS], ty[PERTURB_TAPS];
};
// tile_rows: 0 (the launcher's choice), 8 or 32 rows per tile; member_shares: 0 (the launcher's choice) or
// 1 .. 65535 workgroups per tile, clipped to the forecast members.  The result depends on neither.
hipError_t ens_launch_perturb(const EnsGeom& g, double* f, const PerturbArgs& a, bool centered, hipStream_t st,
                              int tile_rows = 0, int member_shares = 0);

// the relaxation of csim_ensemble_prior_capture / csim_ensemble_relax (ensemble_relax.hip), one launch each; forecast
// member k is forecast_member(k, truth_member) of ensemble_cell.hpp (truth_member = B: none skipped),
// 2 <= forecast <= ASSIM_MAX_MEMBERS.
// sb: nx * ny values, interior cell (i, j) at (j - 1) nx + (i - 1).
// sb = sqrt(v) of mv(x) on every interior cell
hipError_t ens_launch_relax_capture(const EnsGeom& g, const double* f, int forecast, int truth_member, double* sb,
                                    hipStream_t st);
// RTPS: x_k <- x_k + fac (x_k - m) where fac != 0; factor (null: not wanted): dense (ny+2) x (nx+2), gets fac on
// the interior
hipError_t ens_launch_relax_spread(const EnsGeom& g, double* f, int forecast, int truth_member, double alpha,
                                   const double* sb, double* factor, hipStream_t st);
// RTPP: x_k <- x_k + alpha ((xb_k - m_b) - (x_k - m)); fb: the captured copy of a whole ping-pong buffer, addressed as f
hipError_t ens_launch_relax_pert(const EnsGeom& g, double* f, const double* fb, int forecast, int truth_member,
                                 double alpha, hipStream_t st);

// the observation network of csim_obs_network_* (ensemble_obs.hip).  Device arrays in plan order but for `pos`, `bg`
// and `post`, which go by input index; the analysis reads i, j, idx, y and r through an AssimArgs.
constexpr int OBS_CHUNK = 256;       // input indices per chunk of the log's sums
constexpr int OBS_CYCLE_FIELDS = 13; // doubles of a csim_obs_cycle: n, has_truth and the 11 sums
constexpr int OBS_SUMS = 11;
constexpr int OBS_MAX_TAPS = 64;     // CSIM_OBS_MAX_TAPS: taps of one linear observation
struct ObsArgs {
    int nobs;
    const int* i;
    const int* j;
    const int* idx;               // input index of a plan position
    const int* pos;               // plan position of an input index
    const double* r;
    const double* sr;             // sqrt(r)
    double* y;
    double* xt;
    const double* bg;             // 2 per input index: hb, vb
    const double* post;           // 2 per input index: ha, va
    double* part;                 // OBS_SUMS per chunk: T_c
    const int* tstart;            // the taps, as in AssimArgs; null: point observations
    const int* toff;
    const double* tw;
};
// screening (csim_obs_network_set_active, csim_ensemble_assimilate_screened); mask and status in plan order
constexpr int OBS_SCREEN_FIELDS = 3; // doubles of a csim_obs_screen_cycle, and counts per chunk: used, inactive, rejected
struct ObsScreen {
    const unsigned char* mask;    // 1: active; null: all active
    unsigned char* status;        // CSIM_OBS_USED / _INACTIVE / _REJECTED of the analysis that follows
    const double* bg;             // 2 per input index: hb, vb (read only with check)
    int check;                    // tol > 0: the background check is made
    double k2;                    // tol * tol, rounded on the host
    int* cnt;                     // OBS_SCREEN_FIELDS per chunk: the counts of the last recorded, screened analysis
};
// y and xt of every observation from member `member` (with taps: xt = h of that member); noise: y = xt + sr z, z the deviate of (seed, draw, input index)
hipError_t ens_launch_obs_observe(const EnsGeom& g, const double* f, const ObsArgs& a, int member, unsigned seed_lo,
                                  unsigned seed_hi, unsigned draw, bool noise, hipStream_t st);
// the chunk sums T_c, then their fold in chunk order into the record `slot` (OBS_CYCLE_FIELDS doubles)
hipError_t ens_launch_obs_cycle(const ObsArgs& a, bool has_truth, double* slot, hipStream_t st);
// the status of every observation from the mask and, with s.check, (y, hb, vb, r)
hipError_t ens_launch_obs_screen(const ObsArgs& a, const ObsScreen& s, hipStream_t st);
// ens_launch_obs_cycle of a screened analysis: the terms of observations that are not used are +0, slot[0] is the
// number used, and `sslot` (OBS_SCREEN_FIELDS doubles) gets the three counts
hipError_t ens_launch_obs_cycle_screened(const ObsArgs& a, const ObsScreen& s, bool has_truth, double* slot,
                                         double* sslot, hipStream_t st);
// (nobs, 0, 0) into each of `cycles` records of a screen log: what a cycle that is not screened leaves there
hipError_t ens_launch_obs_screen_log_fill(double* slog, int cycles, int nobs, hipStream_t st);

// ensemble space (ensemble_space.hip; csim_ensemble_gram, _project, _transform): the M x M space spanned by the forecast
// members' perturbations p_k (x_k less the cell's mean when centered, x_k itself otherwise).
// The limits ESPACE_MAX_MEMBERS and DOT_MAX_FIELDS, the Gram sum's plan (gram_classes, gram_pairs) and GRAM_FORMS:
// gram_plan.hpp.
constexpr int PROJECT_FORMS = 1;  // project_form 1: the members of a cell in LDS whatever M
// G (M x M, device) from the members; partial: gram_classes x gram_pairs doubles.  form: 0 (the launcher's choice)
// or 1 .. GRAM_FORMS; the result does not depend on it
hipError_t ens_launch_gram(const EnsGeom& g, const double* f, int forecast, int truth_member, bool centered,
                           double* partial, double* G, int form, hipStream_t st);
// out_r = sum_k p_k W[k K + r] on every cell of the dense layout (ny+2) x (nx+2): K dense fields.  W on the device.
// form: 0 or 1 .. PROJECT_FORMS
hipError_t ens_launch_project(const EnsGeom& g, const double* f, int forecast, int truth_member, bool centered, int K,
                              const double* W, double* out, int form, hipStream_t st);
// x_r <- (m + sum_k p_k wbar[k]) + sum_k p_k W[k M + r] (centered; wbar null: m) or sum_k p_k W[k M + r] on every
// interior cell of the forecast members, in place.  gate (device, may be null): the status word of an EtkfRecord; the
// kernel writes nothing when it reads ETKF_NONFINITE or ETKF_SKIP there
hipError_t ens_launch_transform(const EnsGeom& g, double* f, int forecast, int truth_member, bool centered,
                                const double* W, const double* wbar, int form, hipStream_t st,
                                const int* gate = nullptr);

// the adjoint of the projection (ensemble_dot.hip; csim_ensemble_dot): out[k K + r] = sum over the interior of p_k f_r,
// M x K on the device, in the order of the Gram sum.  fields (device): K fields of nx ny values, interior cell
// e = (j - 1) nx + (i - 1) of field r at r nx ny + e; partial: ens_dot_partial_doubles doubles.  One geometry
size_t ens_dot_partial_doubles(const EnsGeom& g, int forecast, int K);
hipError_t ens_launch_dot(const EnsGeom& g, const double* f, int forecast, int truth_member, bool centered, int K,
                          const double* fields, double* partial, double* out, hipStream_t st);
// the forecast impact without localisation (ensemble_dot.hip; csim_ensemble_obs_impact_global): J_o of every
// observation, by input index, from a capture (ImpactCapture, plan order) and g (M values, device)
struct ImpactGlobalArgs {
    int nobs;
    int forecast;                 // M of the capture, 2 .. ESPACE_MAX_MEMBERS
    const int* idx;
    const unsigned char* snap;
    const double* pert;
    const double* dn;
    const double* g;
};
hipError_t ens_launch_obs_impact_global(const ImpactGlobalArgs& a, double* out, hipStream_t st);

// the observation-space Gram matrix of csim_ensemble_obs_gram (ensemble_obsgram.hip): A = Z^T Z, (M + 1) x (M + 1), of
// the normalised observation-space perturbations of a network, and the members' sums of squared normalised departures.
// Device arrays in plan order.  An observation is used iff flag is null or flag[q] == used: the mask (1: active) of
// the stand-alone call, the status bytes (0: CSIM_OBS_USED) of an analysis.
struct ObsGramArgs {
    int nobs;
    int forecast;                 // M
    int truth_member;             // t, or B (no member skipped)
    const int* i;
    const int* j;
    const double* y;
    const double* sr;             // sqrt(r)
    const unsigned char* flag;
    int used;
    const int* tstart;            // the taps, as in AssimArgs; null: point observations
    const int* toff;
    const double* tw;
    // csim_ensemble_obs_gram_held: M doubles per plan position, read as h_k in place of the gather (then i, j and the
    // taps are not read, and truth_member plays no part); null: gather.  Last, as the taps are in AssimArgs
    const double* rows;
};
// doubles of `partial` for a call: per class the packed upper triangle of A, M sums of loglik and one count
size_t ens_obs_gram_partial_doubles(int forecast, int nobs);
// out (device): A, then M values of loglik (written only with want_loglik), then the number of used observations as
// one long long.  form: 0 (the launcher's choice) or 1 .. GRAM_FORMS; the result does not depend on it
hipError_t ens_launch_obs_gram(const EnsGeom& g, const double* f, const ObsGramArgs& a, bool want_loglik,
                               double* partial, double* out, int form, hipStream_t st);

// held observation-space rows (ensemble_held.hip; csim_obs_network_hold, csim_ensemble_assimilate_etkf_held): M doubles
// per plan position, [plan position][member], the layout of the local analysis's priors.
// h_k of `count` observations from the current members: block b serves plan position list[b] (list null: b).  The
// AssimArgs as for ens_launch_local_prior; status is not read
hipError_t ens_launch_obs_hold(const EnsGeom& g, const double* f, const AssimArgs& a, const int* list, int count,
                               double* rows, hipStream_t st);
// mv of csim_ensemble_relax over the M values of every row, 2 per input index (idx: the input index of a position)
hipError_t ens_launch_held_mv(const double* rows, int nobs, int M, const int* idx, double* out, hipStream_t st);
// every row as one cell's M members under ens_launch_transform(centered), in place; gate as there
hipError_t ens_launch_held_transform(double* rows, int nobs, int M, const double* W, const double* wbar, hipStream_t st,
                                     const int* gate = nullptr);
// ens_launch_obs_observe for the `count` plan positions list[0 .. count)
hipError_t ens_launch_obs_observe_list(const EnsGeom& g, const double* f, const ObsArgs& a, const int* list, int count,
                                       int member, unsigned seed_lo, unsigned seed_hi, unsigned draw, bool noise,
                                       hipStream_t st);

// the device eigensolver and the ETKF's weights on the device (sym_eigen_device.hip), in the round-robin order of
// include/csim.h.  `batch` matrices of n x n (rows lda doubles apart, a_stride doubles from one to the next), one
// workgroup each; work: 2 n^2 doubles per matrix; lambda: n, V: n x n per matrix; info: sweeps and status (EIGEN_*)
// per matrix.  A matrix with a non-finite entry gets NaN in lambda and V.  form: 0 (by n) or 1 .. EIGEN_FORMS of
// sym_eigen.hpp; the result does not depend on it
hipError_t ens_launch_sym_eigen(int n, int batch, const double* A, int lda, long a_stride, double* work,
                                double* lambda, double* V, int* info, int form, hipStream_t st);
// what a device ETKF leaves for csim_ensemble_etkf_info, followed by gamma (M doubles)
struct EtkfRecord {
    double dfs, chi2;
    long long n_used;
    int sweeps, status;  // ETKF_*
};
constexpr int ETKF_OK = 0, ETKF_NONFINITE = 1, ETKF_NOT_CONVERGED = 2, ETKF_SKIP = 3;
// W (M x M) and wbar of csim_etkf_weights_ordered(order = round robin) from the output of ens_launch_obs_gram (A) and
// of ens_launch_sym_eigen on its leading M x M block (lambda, V, info); the record and gamma.  status: ETKF_NONFINITE
// when an entry of A is not finite, else ETKF_SKIP with no used observation and inflation 1, else the solver's
hipError_t ens_launch_etkf_weights(int M, const double* A, const double* lambda, const double* V, const int* info,
                                   double inflation, double* W, double* wbar, EtkfRecord* rec, double* gamma,
                                   hipStream_t st);

// the LETKF of csim_ensemble_assimilate_letkf: the weights on a lattice of analysis nodes (letkf_nodes.hpp), interpolated
// to the cells.  After ens_launch_local_prior: the node Gram matrices (ensemble_letkf.hip), ens_launch_sym_eigen on them
// where they lie, the weights of every node (sym_eigen_device.hip), and the cell pass (ensemble_letkf.hip).
struct LetkfGramArgs {
    int nax, nay, spacing;        // the lattice: nay x nax nodes, node (a, b) at index b nax + a
    const int* cstart;            // per node, one more than nodes: its candidates are cpos[cstart[g]] .. cpos[cstart[g + 1] - 1]
    const int* cpos;              // plan positions, sorted by input index within a node
    const double* prior;          // M per plan position: h_{o,k}
    double* A;                    // (M + 1)^2 per node
    int* count;                   // per node: |L(g)|
};
// A_g and count_g of every node; the AssimArgs as for ens_launch_local_prior.  form: 0 or 1 .. GRAM_FORMS, as
// ens_launch_obs_gram; the result does not depend on it
hipError_t ens_launch_letkf_gram(const EnsGeom& g, const AssimArgs& a, const LetkfGramArgs& l, int form, hipStream_t st);
// per node: status LETKF_IDLE (count 0) or LETKF_NONFINITE (an entry of A is not finite) with dfs = +0 and sweeps = 0,
// else W (M x M), wbar, dfs of csim_etkf_weights_ordered(M, A, 1.0, round robin) from the solver's lambda, V and info
// (sweeps, status per node), with the solver's sweeps and LETKF_OK or LETKF_NOT_CONVERGED
hipError_t ens_launch_letkf_weights(int M, int nodes, const double* A, const double* lambda, const double* V,
                                    const int* info, const int* count, double* W, double* wbar, double* dfs, int* sweeps,
                                    int* status, hipStream_t st);
struct LetkfCellArgs {
    int nax, nay, spacing;
    const double* W;              // M^2 per node
    const double* wbar;           // M per node
    const int* status;            // per node
};
// the cell pass: every interior cell of the forecast members from the weights of its four nodes, in place.
// form: 0 or 1 .. LETKF_FORMS of letkf_nodes.hpp; the result does not depend on it
hipError_t ens_launch_letkf_cells(const EnsGeom& g, double* f, int M, int t, const LetkfCellArgs& l, int form,
                                  hipStream_t st);

// the rank histogram's tie-break: splitmix64's finaliser of the interior index g; a cell with `eq` members equal to the
// truth goes to bin lt + mix(g) mod (eq + 1)
__host__ __device__ inline unsigned long long verify_mix(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace csim
