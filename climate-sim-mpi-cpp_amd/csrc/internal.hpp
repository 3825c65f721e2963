// internal.hpp — shared declarations of the HIP engine behind include/csim.h.
//
// Device layout of a Field (MI355X-first, not the host layout): rows are padded to a pitch
// so that the FIRST INTERIOR column (i = 1) of every row starts on a 128-byte boundary and a
// 64-lane wavefront reading 2 doubles per lane covers exactly 8 full 128-byte lines:
//
//     element (i, j), 0 <= i <= nx+1, 0 <= j <= ny+1   ->   view[j * pitch + (LPAD - 1) + i]
//
//     | 15 unused | ghost i=0 | interior i=1..nx (128-B aligned) | ghost i=nx+1 | pad ... |
//
// `view` points GHOST_EXTRA rows into the allocation: rows -6..-1 and ny+2..ny+7 (and the pad
// columns left of i = 0 / right of i = nx+1) exist as device-only ghost layers, which the
// multi-step-per-pass sweeps read (as halo data on neighbour sides, as don't-care otherwise).
//
// pitch = LPAD + round_up(nx + 1, 128) + 128 doubles; for nx = 16384 that is 16656 doubles =
// 133248 B, an odd multiple of 128 B, so vertically adjacent rows do not alias onto one HBM
// channel.  Pads are zero and never written.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <string>

#include "csim.h"
#include "sweep_plan.hpp"  // WAVE_COLS, MAX_FUSE, cdiv, the tile plan of the overlapped-strip sweep (host arithmetic)

namespace csim {

constexpr int LPAD = 16;  // doubles in front of the first interior column

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int pitch_for(int nx) { return LPAD + round_up(nx + 1, WAVE_COLS) + WAVE_COLS; }

int fail(int code, const std::string& msg);

#define CSIM_HIP(expr)                                                                       \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return ::csim::fail(CSIM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// physics constants of one sweep, precomputed on the host exactly as the reference forms them
struct Phys {
    double kdiff;  // dt * D            (reference src/diffusion.cpp:15  "dt * D * lap")
    double mdt;    // -dt               (reference src/advection.cpp:31  "(-dt) * adv")
    double vx, vy;
    double dx, dy;      // divisors of the upwind differences
    double dx2, dy2;    // dx*dx, dy*dy: divisors of the second differences
    double rdx, rdy, rdx2, rdy2;  // exact reciprocals (only used when all four are powers of two)
    int div_mode;       // 0: dx == dy == 1 (x/1 is x)   1: exact reciprocal multiply   2: IEEE divide
                        // 3: option "contract" — the coefficient form below (not bit-identical)
    double a0, aW, aE, aS, aN;  // u' = a0 c + aW W + aE E + aS S + aN N, the same update as one 5-point stencil
    double fast_thr;    // > 0: k_sweepO_dpp may fuse E - 2c into one fma on tiles whose loaded values are all below
                        // this magnitude (no 2c of any level can overflow then); 0: always the plain form
    // power-of-two velocities (option "pow2_v"; make_phys): the advection term as fma(q, g1, g2) and one
    // product with K — 12 instead of 14 operations per cell — on tiles whose loaded values are all exactly zero or at
    // least slow_thr in magnitude, and below p2_hi
    double slow_thr;    // > 0: the form is enabled for these parameters (the screen's lower bound L); 0: off
    double p2_hi;       // the screen's upper bound in that body: fast_thr lowered so that no product with q can overflow
    double p2_q, p2_k;  // q = (vx/dx)/(vy/dy) or its reciprocal, K = (-dt) * the velocity factored out (see cell)
};
Phys make_phys(double dx, double dy, double D, double dt, double vx, double vy, bool contract = false);
// Screen lease: what a whole field has to satisfy NOW so that, R + MAX_FUSE steps on, every value still
// passes the screen of the interior bodies — pure host arithmetic on a Phys (api.cpp).
//   M_req  max|u| <= M_req keeps every value below p2_hi (fast_thr where the 12-operation form is off); 0: no lease
//   m_req  with all five stencil coefficients positive and the field of one sign: min|u| >= m_req keeps every value
//          at or above 2 slow_thr; 0: no lease of the 12-operation body for these parameters
//   eta    the relative loss of one computed update against the exact one that m_req allows for (32 g eps / a_min)
struct LeaseBounds {
    double M_req = 0.0, m_req = 0.0, eta = 0.0;
};
LeaseBounds lease_bounds(const Phys& p, long R);
// upwind-sign flavour of these parameters, 3 * cx + cy with per axis 0: v < 0, 1: v >= 0, 2: v == 0 on a screened run
// (fast_thr > 0 and dx, dy without IEEE division): which k_sweepO_dpp<., ., SX, SY> / k_ensemble_sweepO<., ., SX, SY>
// a launch runs, and the class an ensemble member is launched with (ENS_CLASSES of them)
inline int sign_class(const Phys& p) {
    const bool screened = p.div_mode <= 1 && p.fast_thr > 0.0;
    const int cx = screened && p.vx == 0.0 ? 2 : (p.vx >= 0.0 ? 1 : 0);
    const int cy = screened && p.vy == 0.0 ? 2 : (p.vy >= 0.0 ? 1 : 0);
    return 3 * cx + cy;
}

// kernel variants of the fused sweep (option "variant")
enum { VAR_AUTO = 0, VAR_DPP = 1, VAR_LDS = 2, VAR_NAIVE = 3 };

struct SweepCfg {
    int variant = VAR_AUTO;
    int rows_per_chunk = 0;  // 0 = auto
    int tuned_rows = 0;      // auto mode: rows per chunk found by the stepper's on-device trial (0 = heuristic)
    int lds_bytes = 0;       // dynamic LDS requested per workgroup of the fused sweep: an occupancy limiter
                             // (41 KB -> 3 workgroups per CU instead of 4), the kernel never touches it
    int prefetch = 0;        // 0 = auto (rows kept in flight per wavefront)
    int xcd_swizzle = 1;
    int tail_split = 1;        // fused launches of two or more rounds of wavefronts end with a region of half-height
                               // chunks (see Tiling); 0 off, 2 experiment (half + quarter height)
    int frame_rows = 0;        // multi-rank pass: chunk height of the frame's side strips (0 = as thin as the bands)
    int wide = 0;              // whole-field launch: wide strips wherever one fits (set per launch, passes.cpp: wide_wanted)
};
// what the tile plan (sweep_plan.hpp) of one launch_sweepO with these settings is made from, and the plan
inline SweepPlanIn plan_in_sweepO(int nx, int ny, int T, const Phys& p, const SweepCfg& cfg, const int kind[4], int part) {
    return SweepPlanIn{nx, ny, T, p.div_mode, {kind[0], kind[1], kind[2], kind[3]}, part,
                       cfg.rows_per_chunk, cfg.tuned_rows, cfg.tail_split, cfg.frame_rows, cfg.wide};
}
inline SweepPlan plan_sweepO(int nx, int ny, int T, const Phys& p, const SweepCfg& cfg, const int kind[4], int part) {
    return sweep_plan(plan_in_sweepO(nx, ny, T, p, cfg, kind, part));
}

// ---- kernel launchers (kernels.hip; launch_sweepO's templates: sweepO.hpp, its tile plan: sweep_plan.cpp) ----
// All pointers are device pointers in the padded layout above.
hipError_t launch_sweep(const double* in, double* out, int nx, int ny, int pitch, const Phys& p,
                        const SweepCfg& cfg, hipStream_t st);
// T = 2..7 fused time steps per pass (overlapped strips) over the tiles of `plan` (plan_sweepO with the same p, cfg
// and kind; nx, ny and T are the plan's).  kind[s] = CSIM_BC_* on physical sides, 3 on neighbour sides; the plan's
// part: 0 = every tile, 1 = frame tiles only, 2 = all but the frame tiles.
// fin_lines (last pass of a run, all four or nullptr): per side the level T-1 line the final ghost
// fill needs — see FinLines in sweep_core.hpp
// part 3 = frame and bulk in ONE grid (frame tiles dispatched first); with `sync` the frame wavefronts
// count themselves on sync->counter and the last one stores sync->pass into sync->flag (signal memory a
// stream can wait on with hipStreamWaitValue64), see k_sweepO_dpp
struct FrameSync {
    unsigned* counter = nullptr;
    unsigned long long* flag = nullptr;
    unsigned long long pass = 0;
    unsigned nframe = 0;  // filled in by the launcher, from the plan
    int fence = 0;        // 0 write-through result stores + drain (default), 1 plain stores + agent-scope fence per
                          // wavefront (slow: +40 us per pass)
    int prio = 1;         // frame wavefronts raise their issue priority
    // direct faces (face_depth > 0): the frame wavefronts also copy the cells that form the faces of the NEXT pass
    // (depth face_depth, k_halo2_pack's layout) straight into the send buffers; nullptr = no peer in that direction
    double* face[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int face_depth = 0;
};
hipError_t launch_sweepO(const double* in, double* out, int pitch, const Phys& p, const SweepCfg& cfg,
                         const int kind[4], double value, const SweepPlan& plan, hipStream_t st,
                         double* const fin_lines[4] = nullptr, const FrameSync* sync = nullptr,
                         const unsigned* lease = nullptr);  // lease: the verdict word of launch_lease below, or nullptr
// depth with the lowest measured cost per time step (tools/depth_ab.py, profiles/r02_depth_ab.jsonl): 7 on tiles
// of >= 2e8 cells (+0.9 % over 6 at 16384^2 and 32768^2); 6 in between (7 loses 7 % on a 4096 x 8192 tile, which is
// a single round of wavefronts: more overhead rows per chunk and nothing to amortise them); 4 on tiles below
// 1.2e7 cells, where a launch is a fraction of one round and the length of a wavefront's dependent chain
// decides (+17...22 % over 6 at 512^2, 1024^2, 3072^2)
constexpr long BIG_TILE_CELLS = 200000000L;
constexpr long SMALL_TILE_CELLS = 12000000L;
// `still` — the diffusion-only flavour (v == 0: half the arithmetic, so the sweep is HBM-bound and every extra level
// per pass pays): 7 at every size (profiles/r03_diffusion_only_depth.jsonl: +8 % over 6 at 4096^2, +13 % at 8192^2 and 16384^2)
inline int pref_fuse(long tile_cells, bool still = false) {
    if (still) return 7;
    return tile_cells >= BIG_TILE_CELLS ? 7 : (tile_cells > 0 && tile_cells < SMALL_TILE_CELLS) ? 4 : 6;
}
constexpr int GHOST_EXTRA = 6;    // device-only ghost layers beyond the reference's one (= MAX_FUSE-1)
// faces of depth H = 2..7 (8 directions: L R B T BL BR TL TR; nullptr = no neighbour there);
// sizes H*(ny+2) (L,R), H*(nx+2) (B,T), H*H (corners)
hipError_t launch_halo2_pack(const double* f, int nx, int ny, int pitch, int depth,
                             double* const send[8], hipStream_t st);
hipError_t launch_halo2_unpack(double* f, int nx, int ny, int pitch, int depth,
                               double* const recv[8], hipStream_t st);

hipError_t launch_diffusion_only(const double* in, double* out, int nx, int ny, int pitch,
                                 const Phys& p, hipStream_t st);
hipError_t launch_advection_only(const double* in, double* out, int nx, int ny, int pitch,
                                 const Phys& p, hipStream_t st);
hipError_t launch_ring_copy(const double* in, double* out, int nx, int ny, int pitch, hipStream_t st);
hipError_t launch_fill(double* f, int nx, int ny, int pitch, double v, hipStream_t st);

struct GhostArgs {
    int bc[4];
    int phys[4];          // side is a physical edge (no neighbour)
    double value;
    const double* recv[4];  // per side: staged halo from the neighbour (nullptr on physical sides)
    const double* adj[4];   // per side: adjacent interior line to read instead of the field (nullptr = the field)
};
// boundary fill (+ unpack of received halos) written to `a` and, when b != nullptr, to `b` too
// ext_depth > 0 additionally continues each physical Dirichlet/Neumann edge over that many halo
// cells of an adjacent neighbour side (needed by fused passes across ranks; reads halo cells a
// preceding launch_halo2_unpack wrote)
hipError_t launch_ghost_fill(double* a, double* b, int nx, int ny, int pitch, const GhostArgs& g,
                             hipStream_t st, int ext_depth = 0);
// updated values of the four edge lines of the NEXT field, computed from `in` and written
// straight into the send staging buffers (nullptr = side not needed)
hipError_t launch_edge_pack(const double* in, int nx, int ny, int pitch, const Phys& p,
                            double* const send[4], hipStream_t st);
// plain pack of the current edge lines (used by csim_stepper_exchange_halos)
hipError_t launch_pack(const double* in, int nx, int ny, int pitch, double* const send[4],
                       hipStream_t st);
hipError_t launch_gaussian(double* f, int nx, int ny, int pitch, int x_off, int y_off, int nxg,
                           int nyg, double dx, double dy, double A, double sigma_frac,
                           double xc_frac, double yc_frac, hipStream_t st);

// reductions (k_reduce<KIND>, k_checksum of kernels.hip): partial results per block in `scratch`, finished on the host
// (fold_partials, fold_checksum of api.cpp).  A window of `rows` rows takes G = reduce_blocks(rows, cap) blocks per
// member; the partial of member m's block b is scratch[m * G + b], the maxima of minmax follow all the minima.
constexpr int REDUCE_BLOCKS = 1024;  // cap of a Field or Stepper: scratch >= 2 * REDUCE_BLOCKS doubles
inline int reduce_blocks(int rows, int cap) { return rows < cap ? rows : cap; }
struct Members {  // the fields one launch reduces: one Field or Stepper, or an ensemble's members
    int count = 1;
    long slab = 0;  // doubles from one member to the next
    int cap = REDUCE_BLOCKS;
};
hipError_t launch_minmax(const double* f, int nx, int ny, int pitch, double* scratch, hipStream_t st,
                         const Members& mb = {});
hipError_t launch_sum(const double* f, int nx, int ny, int pitch, double* scratch, hipStream_t st,
                      const Members& mb = {});
hipError_t launch_linf(const double* a, const double* b, int nx, int ny, int pitch, double* scratch,
                       hipStream_t st);
// k_reduce<3>, the screen lease's verdict: over rows 0..ny+1 and columns 0..nx+1 (ring cells told from interior ones)
// max|u|, min|u| over non-zero values and the sign / zero / non-finite flags; the block that finishes last folds the
// partials and stores the verdict into lease[0] — bit 0 (LEASE_FAST): max|u| <= M_req and nothing non-finite; bit 1
// (LEASE_P2): also m_req > 0, min|u| >= m_req, the interior strictly of one sign and no ring value of the other sign
// or a zero of the other sign.  lease[1] is the kernel's ticket counter (zero between launches).  Nothing comes back to the host.
constexpr int LEASE_BLOCKS = 512;  // three partials per block in the same scratch
hipError_t launch_lease(const double* f, int nx, int ny, int pitch, double* scratch, double M_req, double m_req,
                        unsigned* lease, hipStream_t st);
// max that keeps a NaN (fmax drops one): every stage of the L-inf reduction — lane, wave, block (k_reduce<2>) and the
// host merge (fold_partials) — goes through it, so max |a-b| is NaN as soon as one |a-b| is
__host__ __device__ __forceinline__ double max_nan(double r, double d) { return (d > r || d != d) ? d : r; }
// position-weighted 64-bit checksum of the interior (k_checksum): reduce_blocks(ny, cap) u64 partials per member
hipError_t launch_checksum(const double* f, int nx, int ny, int pitch, long x_off, long y_off, long nx_global,
                           double* scratch, hipStream_t st, const Members& mb = {});

}  // namespace csim

// ---- opaque handle types -------------------------------------------------------------------
struct csim_field {
    int nx = 0, ny = 0, halo = 1;
    double dx = 1.0, dy = 1.0;
    int pitch = 0;
    double* alloc = nullptr;    // (ny + 2 + 2 * GHOST_EXTRA) * pitch doubles
    double* d = nullptr;        // view: alloc + GHOST_EXTRA * pitch, i.e. row j = 0 of the reference layout
    double* scratch = nullptr;  // reduction partials
    size_t bytes() const {
        return sizeof(double) * static_cast<size_t>(ny + 2 + 2 * csim::GHOST_EXTRA) * pitch;
    }
};
