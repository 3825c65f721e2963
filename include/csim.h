/* include/csim.h — C ABI of the MI355X-native advection–diffusion stepper.
 *
 * This is the drop-in boundary for ONE hot path of antoniorizzoeng/climate-sim-mpi-cpp:
 * the per-time-step sequence
 *     exchange_halos -> apply_boundary -> copy -> diffusion_step -> advection_step -> swap
 * (reference src/main.cpp:101-109).  The reference has no FFI/plugin layer: its boundary is
 * the set of C++ free functions and structs in include/{field,decomp,halo,boundary,diffusion,
 * advection,stability}.hpp.  Each entry point below names the reference interface it replaces.
 * The C++ mirror of those headers (same names and signatures) lives in include/climate/ and
 * calls only this ABI.
 *
 * Conventions
 *   - every function returns 0 (CSIM_OK) or a CSIM_ERR_* code; csim_last_error() gives the text
 *     (thread-local).  No C++ types, no exceptions cross this boundary.
 *   - host arrays use the reference layout (reference src/field.cpp:20-25): row-major, ghost
 *     ring included, element (i,j) at host[j*(nx+2*halo)+i], i contiguous.  Only halo==1 is
 *     supported, like the reference driver (src/main.cpp:65); other values give CSIM_ERR_ARG.
 *   - sides are ordered left(x-), right(x+), bottom(y-), top(y+) everywhere.
 *   - all arithmetic is IEEE fp64 in the reference's association order with no FMA
 *     contraction, so results are bit-identical to the reference CPU path.
 *   - there is NO CPU fallback: without a usable gfx950 device the calls fail with CSIM_ERR_HIP.
 *   - a handle is not thread-safe; use one stepper per GPU (one process per GPU).
 */
#ifndef CSIM_H
#define CSIM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSIM_ABI_VERSION 1

enum {
    CSIM_OK = 0,
    CSIM_ERR_ARG = 1,         /* bad argument (maps to std::out_of_range / std::runtime_error) */
    CSIM_ERR_HIP = 2,         /* a HIP runtime call failed, or no device */
    CSIM_ERR_RCCL = 3,        /* an RCCL call failed */
    CSIM_ERR_STATE = 4,       /* call sequence error (e.g. multi-rank run before comm init) */
    CSIM_ERR_UNSUPPORTED = 5,
    CSIM_ERR_TIMEOUT = 6      /* csim_stepper_sync with option "sync_timeout_ms": the streams did not drain in time */
};

/* reference include/boundary.hpp:5  enum class BCType { Dirichlet, Neumann, Periodic } */
enum { CSIM_BC_DIRICHLET = 0, CSIM_BC_NEUMANN = 1, CSIM_BC_PERIODIC = 2 };
enum { CSIM_LEFT = 0, CSIM_RIGHT = 1, CSIM_BOTTOM = 2, CSIM_TOP = 3 };

#define CSIM_NO_NEIGHBOR (-1)   /* stands for MPI_PROC_NULL */
#define CSIM_UNIQUE_ID_BYTES 128

typedef struct csim_field csim_field;     /* device mirror of reference `struct Field`       */
typedef struct csim_stepper csim_stepper; /* the time-loop engine (reference main.cpp:93-118) */

/* reference include/decomp.hpp:4-17 `struct Decomp2D` without the MPI communicator */
typedef struct csim_decomp {
    int size, rank;
    int dims[2];    /* dims[0] splits x (the contiguous axis), dims[1] splits y */
    int coords[2];
    int nbr[4];     /* left,right = nbr_lr[0..1]; bottom,top = nbr_du[0..1]; CSIM_NO_NEIGHBOR */
    int nx_global, ny_global;
    int nx_local, ny_local;
    int x_offset, y_offset;
} csim_decomp;

/* ---- library / device ------------------------------------------------------------------ */
const char* csim_last_error(void);
int csim_abi_version(void);
int csim_device_count(int* count);
int csim_set_device(int device);           /* one process per GPU: call once with LOCAL_RANK */
int csim_device_name(char* buf, size_t n); /* gcnArchName of the current device */

/* ---- host-side scalars ------------------------------------------------------------------ */
/* reference include/stability.hpp:5-16  double safe_dt(dx,dy,vx,vy,D) */
double csim_safe_dt(double dx, double dy, double vx, double vy, double D);
/* host arithmetic only: the screen and the constants of the stepper option "pow2_v" for these parameters —
 * out[0] = L, the smallest non-zero magnitude a tile may load and still take the 12-operation body (0 = the form is off
 * for these parameters), out[1] = its upper bound, out[2] = q, out[3] = K */
int csim_pow2_velocity_screen(double dx, double dy, double D, double dt, double vx, double vy, double out[4]);
/* host arithmetic only: the bounds of the stepper option "screen_lease" for these parameters and a lease of R steps —
 * out[0] = M_req: max|u| <= M_req now keeps every value below the screen's upper bound for R + 7 steps (0 = no lease);
 * out[1] = m_req: with all five stencil coefficients positive and a field of one sign, min|u| >= m_req now keeps
 * every value at or above twice the L of csim_pow2_velocity_screen for R + 7 steps (0 = the 12-operation body is not
 * leased for these parameters); out[2] = eta, the relative loss per step the lower bound allows for rounding;
 * out[3] = a0, the centre coefficient (min|u| shrinks by at most a0 (1 - eta) per step).  DESIGN.md section 4 */
int csim_screen_lease_bounds(double dx, double dy, double D, double dt, double vx, double vy, long R, double out[4]);
/* reference src/decomp.cpp:5-34  Decomp2D::init(comm, nx_global, ny_global), MPI-free:
 * MPI_Dims_create(size,2) + MPI_Cart_create(periods 0,0, reorder 0) are re-derived. */
int csim_decomp_init(int size, int rank, int nx_global, int ny_global, csim_decomp* out);
/* The halo exchange of one rank as an ordered message list (pure host arithmetic, no GPU): what
 * the stepper posts inside ONE ncclGroupStart/End — replaces the <= 8 MPI_Isend/Irecv + MPI_Waitall of
 * reference src/halo.cpp:28-46.  depth 1: the four edge lines (ny / nx doubles, interior span);
 * depth 2..7 (fused passes): faces of that depth in 8 directions 0..7 = left, right, bottom, top,
 * bottom-left, bottom-right, top-left, top-right (depth*(ny+2), depth*(nx+2), depth*depth doubles).
 * sends[k].dir = the direction the face leaves in; recvs[k].dir = the direction it arrives FROM.  RCCL
 * matches the messages of a pair of ranks in posting order, so for every pair (a, b) the k-th send
 * of a to b must be the k-th receive b posts for a: tests/test_exchange_plan.py checks exactly that
 * for every rank pair of 2x1 ... 4x2 process grids at every depth. */
typedef struct csim_msg {
    int peer;    /* rank */
    int dir;     /* 0..7 */
    long count;  /* doubles */
} csim_msg;
int csim_exchange_plan(const csim_decomp* dec, int depth, csim_msg sends[8], int* nsend, csim_msg recvs[8],
                       int* nrecv);

/* ---- Field (reference include/field.hpp:5-21, src/field.cpp:6-31) ------------------------ */
int csim_field_create(int nx, int ny, int halo, double dx, double dy, csim_field** out); /* zero-filled */
int csim_field_destroy(csim_field* f);
int csim_field_upload(csim_field* f, const double* host_with_ghosts);
int csim_field_download(const csim_field* f, double* host_with_ghosts);
int csim_field_download_interior(const csim_field* f, double* host_ny_by_nx);
int csim_field_fill(csim_field* f, double value);                 /* Field::fill            */
int csim_field_copy(csim_field* dst, const csim_field* src);      /* std::copy, main.cpp:104 */
int csim_field_swap(csim_field* a, csim_field* b);                /* std::swap, main.cpp:109 */
/* wavefront-level reductions.  minmax spans the whole array, ghosts included, like
 * reference src/main.cpp:73-77; sum/linf span the interior.  NaN and Inf are data:
 *  - minmax skips NaN cells (the reference's std::min_element / max_element skip them too, unless
 *    the NaN is element 0); an array of nothing but NaN gives (+inf, -inf); +-Inf are values;
 *    +0 and -0 compare equal, either may be returned.  csim_stepper_minmax and
 *    csim_ensemble_minmax follow the same rule.
 *  - sum carries them as IEEE addition does (one NaN -> NaN; +Inf -> +Inf; +Inf and -Inf -> NaN).
 *    Its order of additions is fixed, so the same field gives the same bits on every call;
 *    tests/reduce_restatement.py restates it (csim_stepper_sum, csim_ensemble_sum likewise).
 *  - linf_diff is max |a - b| with NaN propagated: if |a - b| is NaN in any interior cell (NaN in
 *    one field, NaN in both, Inf of one sign in both) the result is NaN, as numpy's
 *    abs(a - b).max(); otherwise it is the maximum, +Inf included.  0.0 therefore means that the
 *    interiors are equal number for number (+0 == -0). */
int csim_field_minmax(const csim_field* f, double out_min_max[2]);
int csim_field_sum(const csim_field* f, double* out);
int csim_field_linf_diff(const csim_field* a, const csim_field* b, double* out);

/* ---- the operators at the reference's own granularity ------------------------------------ */
/* reference src/boundary.cpp:12-54  apply_boundary(f, dec, bc, value); is_physical[s] != 0
 * stands for "neighbour on side s is MPI_PROC_NULL". */
int csim_apply_boundary(csim_field* f, const int bc[4], const int is_physical[4], double value);
/* reference src/diffusion.cpp:3-26  diffusion_step(u, out, D, dt) (interior + ring copy) */
int csim_diffusion_step(const csim_field* u, csim_field* out, double D, double dt);
/* reference src/advection.cpp:5-34  advection_step(u, out, vx, vy, dt) (accumulates) */
int csim_advection_step(const csim_field* u, csim_field* out, double vx, double vy, double dt);
/* copy + diffusion_step + advection_step in ONE sweep (reference src/main.cpp:104-107):
 * out := u everywhere, then the fused update on the interior. */
int csim_fused_step(const csim_field* u, csim_field* out, double D, double dt, double vx, double vy);

/* ---- the time loop (reference src/main.cpp:93-118 minus I/O) ------------------------------ */
int csim_stepper_create(const csim_decomp* dec, double dx, double dy, const int bc[4],
                        double bc_value, csim_stepper** out);
int csim_stepper_destroy(csim_stepper* s);
/* multi-GPU: RCCL communicator for the halo exchange (replaces MPI in reference src/halo.cpp).
 * rank 0 calls csim_comm_unique_id, ships the 128 bytes to the other ranks by any means
 * (MPI_Bcast, torch.distributed store, file), then every rank calls csim_stepper_comm_init. */
int csim_comm_unique_id(void* id, size_t nbytes);
int csim_stepper_comm_init(csim_stepper* s, const void* id, size_t nbytes);
/* a second stepper of the SAME rank borrows `owner`'s communicator (small parity cases beside the production tile
 * without paying for another communicator); owner must outlive s, and only one of them may have an exchange in
 * flight at a time (sync one before running the other) */
int csim_stepper_comm_share(csim_stepper* s, csim_stepper* owner);
int csim_stepper_upload(csim_stepper* s, const double* host_with_ghosts);   /* local tile */
int csim_stepper_download(csim_stepper* s, double* host_with_ghosts);
int csim_stepper_download_interior(csim_stepper* s, double* host_ny_by_nx);
/* snapshot without stalling the loop (reference src/io.cpp:402-424 packs + writes inside the step
 * loop, src/main.cpp:96-99): _begin enqueues a device-side copy of the current interior and an
 * asynchronous D2H into a pinned buffer on a third stream and returns at once; keep calling
 * csim_stepper_run, then _wait for the ny_local x nx_local row-major data (valid until the next
 * _begin). */
int csim_stepper_snapshot_begin(csim_stepper* s);
int csim_stepper_snapshot_wait(csim_stepper* s, const double** host_interior);
/* gaussian hotspot written on the device (reference src/init.cpp:12-33) */
int csim_stepper_init_gaussian(csim_stepper* s, double A, double sigma_frac, double xc_frac,
                               double yc_frac);
/* External halo transport (option "external_halo"=1), for callers that keep the reference's
 * MPI exchange (src/halo.cpp:28-46) or any other carrier: pack copies the four edge lines of
 * the current field to host buffers (ny doubles for left/right, nx for bottom/top; entries of
 * physical sides are ignored), unpack stages the lines received from the neighbours for the
 * next csim_stepper_run(.., 1).  One step per run call in this mode. */
int csim_stepper_halo_pack(csim_stepper* s, double* const host_send[4]);
int csim_stepper_halo_unpack(csim_stepper* s, const double* const host_recv[4]);
/* deep-face flavour for csim_stepper_run(.., depth) (ONE fused pass of depth = 2..7 steps) in
 * external mode: directions 0..7 = left, right, bottom, top, bottom-left, bottom-right, top-left,
 * top-right; _neighbors gives the peer rank (or CSIM_NO_NEIGHBOR) and the face length in doubles
 * per direction (depth*(ny+2), depth*(nx+2), depth*depth).  The face packed for direction d must be
 * delivered to peers[d], which unpacks it as coming from the opposite direction (d ^ 1 for
 * sides, 11 - d for corners). */
int csim_stepper_fuse_limit(const csim_stepper* s, int* depth); /* deepest pass available (1 = none) */
int csim_stepper_faces_neighbors(const csim_stepper* s, int depth, int peers[8], int lengths[8]);
int csim_stepper_faces_pack(csim_stepper* s, int depth, double* const host_send[8]);
int csim_stepper_faces_unpack(csim_stepper* s, int depth, const double* const host_recv[8]);
/* reference src/halo.cpp:6-50  exchange_halos(u, dec, comm) on the current field */
int csim_stepper_exchange_halos(csim_stepper* s);
/* nsteps x { exchange_halos; apply_boundary; fused sweep; swap }, enqueued without host syncs;
 * internally up to 7 steps share one pass over HBM; the last pass of a call also leaves the ghost
 * ring the reference would (halos / boundary values of the state before the last step) */
int csim_stepper_run(csim_stepper* s, double D, double dt, double vx, double vy, int nsteps);
/* The pass schedule of csim_stepper_run(nsteps) as pure host arithmetic: depths[k] = time steps the k-th
 * HBM pass advances (the first max_depths of *npasses entries).  smallest_tile = min over the decomposition
 * of the local nx, ny (the face depth cannot exceed it; MAX for one rank), tile_cells = nx * ny of a single-rank
 * stepper (>= 2e8 cells prefer depth 7, below 1.2e7 depth 4, else 6) and 0 for a multi-rank one (every pass
 * carries an exchange: depth 6, or 7 where it saves a pass), fuse = the option "fuse".  It depends on these numbers only, so every rank derives the same
 * schedule without communicating. */
int csim_pass_schedule(int nsteps, int smallest_tile, long tile_cells, int fuse, int* depths, int max_depths,
                       long* npasses);
/* the same for a given arithmetic flavour: diffusion_only != 0 = a run with vx == vy == 0 (see option "fused_2c"), whose
 * sweep does half the arithmetic and is HBM-bound: 7 steps per pass at every tile size (csim_pass_schedule = flavour 0) */
int csim_pass_schedule_for(int nsteps, int smallest_tile, long tile_cells, int fuse, int diffusion_only, int* depths,
                           int max_depths, long* npasses);
/* optional, before a timed loop: the one-off rows-per-chunk trial that the first long
 * csim_stepper_run would otherwise do (option "autotune"), and — with automatic pass depths — a trial for every
 * other depth a pass plan may mix in (4..7; read back as "tuned_rows_4" .. "tuned_rows_7"); does not advance the field */
int csim_stepper_tune(csim_stepper* s, double D, double dt, double vx, double vy);
/* measurement helper: keep this GPU under the stepper's own load for about `seconds` WITHOUT advancing the field
 * and without any communication (whole-tile launches of the multi-step sweep into the scratch buffer, like the
 * trial launches of _tune), returning with the GPU idle not later than `seconds` after the call.  For the wait
 * between a cross-rank barrier and a timed region (reference: the MPI_Wtime bracket of src/main.cpp:94,111 has no
 * such wait): a GPU that idles for milliseconds leaves its sustained power state and runs the first launches of
 * the timed region 5-15 % slower.  On a multi-rank stepper these launches (like the trial launches of _tune) read the
 * deep-halo layers as they are — zero after creation, otherwise the faces of an earlier pass — so their duration is
 * that of a real pass only while those values are finite (a NaN there makes "fused_2c" tiles run twice); the field
 * itself is never affected. */
int csim_stepper_keep_warm(csim_stepper* s, double D, double dt, double vx, double vy, double seconds);
/* waits for everything enqueued.  With an RCCL communicator the wait polls ncclCommGetAsyncError, so a failed
 * exchange returns CSIM_ERR_RCCL instead of hanging (the reference's MPI_Waitall, src/halo.cpp:46, aborts through
 * the MPI error handler); option "sync_timeout_ms" > 0 bounds the wait (CSIM_ERR_TIMEOUT). */
int csim_stepper_sync(csim_stepper* s);
/* bit-identity in one number: sum over the local interior of bits(u) * (0x9E3779B97F4A7C15 + 2 g) mod 2^64, g = the
 * cell's global linear index (y_offset + j) * nx_global + x_offset + i.  The values of all ranks of a decomposition
 * add up (mod 2^64) to the checksum of the same global field on one rank, whatever the process grid. */
int csim_stepper_checksum(csim_stepper* s, unsigned long long* out);
int csim_stepper_minmax(csim_stepper* s, double out_min_max[2]);
int csim_stepper_sum(csim_stepper* s, double* out);
/* tuning / measurement knobs; unknown keys give CSIM_ERR_ARG.  Results never depend on them, with ONE
 * exception that is off by default:
 *   "contract"       0 (default): every cell update is evaluated in the reference's own operation order
 *                    without FMA contraction (src/diffusion.cpp:9-16, src/advection.cpp:13-33) -> results
 *                    are bit-identical to the reference.  1 (opt-in): the same update as the 5-point
 *                    stencil a0 c + aW W + aE E + aS S + aN N in FMA form (5 instead of 15 fp64
 *                    operations per cell); rounding differs by a few ulp per step, L_inf vs the reference
 *                    stays far below the 1e-10 tolerance (tests/test_gpu_contract.py).
 *   "fused_2c"       0/1 (default 1), bit-identical either way: the interior body of the multi-step sweep evaluates
 *                    E - 2c and N - 2c as one fma(-2, c, .) each — 2c is exact, so the result is the reference's —
 *                    and every tile screens the values it loads: if one is so large that some 2c of the pass
 *                    could overflow (or is NaN / Inf), the tile is recomputed with the reference's own operation
 *                    sequence (bit-identical for every non-NaN cell, the same cells NaN; the reference does not define NaN
 *                    payloads).  14 instead of 15 fp64 operations per cell.  "fused_2c_active" (read-only): whether
 *                    the last run's parameters allowed it (growth bound per step, see make_phys)
 *                    With vx == vy == 0 (diffusion only, BASELINE configs[1]) the same screened body also leaves out
 *                    the advection term, whose value is then +-0 (7 instead of 14 operations per cell; a loaded -0
 *                    sends the tile to the reference's sequence, because o + (+0) would turn an o of -0 into +0).
 *                    "diffusion_only_active" (read-only): whether the last run swept that way.  One zero component alone:
 *                    its three operations are left out under the same screen (11 per cell)
 *   "pow2_v"         0/1/2 (default 2 = on for tiles of at least 6e7 cells, where it was measured to pay: 16384^2 +8.5 %,
 *                    8192^2 +6.4 %, but 4096 x 8192 -4 % and 4096^2 -17 %; 1 = on wherever the parameters allow), bit-identical
 *                    in every setting: where vx/dx and vy/dy are both non-zero powers of two
 *                    (every shipped configuration: 0.5, 0.25) the same interior body forms the advection term as
 *                    F = fma(q, gx, gy), m = K F with q = (vx/dx)/(vy/dy) and K = (-dt) vy/dy made on the host — products
 *                    with powers of two are exact and commute with rounding — 12 instead of 14 operations per cell.  The
 *                    identity fails only where such a product loses bits in the subnormal range, so the tile's screen
 *                    also requires every loaded value to be exactly zero or at least L in magnitude (about 2^-600 for the
 *                    bench physics, csim_pow2_velocity_screen; derivation: DESIGN.md section 4); other tiles are recomputed
 *                    with the reference's sequence.  Needs "fused_2c"; passes of 2 or 3 steps, edge tiles, IEEE division,
 *                    "contract" and the ensemble keep their bodies.  "pow2_v_active" (read-only): whether the last run's
 *                    parameters and tile size enabled it.  0 restores the 14-operation body everywhere.  Steppers that
 *                    lease their screen ("screen_lease") take the form from 1.6e7 cells on: without the screen it won
 *                    every round at 4096^2, 4096 x 8192 and 8192^2
 *   "screen_lease"   0/1 (default 1), bit-identical either way; single-rank steppers that are not on the external halo
 *                    transport.  What the interior bodies' screens ask of every value of every tile in every pass —
 *                    below the upper bound; for "pow2_v" also non-zero and at least L — is a property of the whole
 *                    field that provably persists: max|u| grows by at most g per step, and with all five stencil
 *                    coefficients positive and a field of one sign min|u| shrinks by at most a0 (1 - eta) per step
 *                    (csim_screen_lease_bounds).  One reduction over the field and its ghost ring,
 *                    enqueued in front of a pass, leaves a verdict in a device word (bit 0: upper bound, bit 1: all of
 *                    it), and for "lease_steps" steps (default 1024) interior tiles of passes of 4..7 steps run the same
 *                    march without the screen.  The host never reads the word; a refused verdict just leaves the
 *                    screened bodies in charge until the renewal.  Upload, init_*, other run parameters and the
 *                    options that change the arithmetic end a lease.  "lease_acquire_after" (default 512): steps a field
 *                    must have been advanced, since it was set or last judged, before a reduction is spent on it —
 *                    short upload / run / download cycles never pay one.  Read-only: "lease_word" (synchronises; for
 *                    tests), "lease_reductions" (reductions enqueued so far)
 *   "wide_strips"    0/1/2 (default 2), bit-identical either way; steppers that lease their screen, with "pow2_v" in
 *                    force and velocities not both negative, at 6 or 7 steps per pass.  The interior between the
 *                    left-most strip, the right-most strips and the thin bottom and top bands is swept in strips of four
 *                    columns per lane (256 loaded columns per wavefront instead of 128): the lane shifts and the
 *                    columns lost to the overlap of neighbouring strips are the same per wavefront, so a wide strip
 *                    issues 14 % fewer instructions per cell update, at two wavefronts per SIMD instead of four.  The
 *                    wide bodies have no screen: the verdict word picks the leased 12-operation body, else the leased
 *                    14-operation one, else the reference's own sequence.  1 = wherever a wide strip fits; 2 = on
 *                    tiles of at least 6e7 cells and only in passes that are handed a verdict word (measured: 16384^2
 *                    +5.5 %, 8192^2 +4 % in every round; 4096 x 8192 within the noise: DESIGN.md section 4).  The chunk
 *                    height of such launches has its own trial ("tuned_rows_wide_6", "tuned_rows_wide_7", read-only).
 *                    "wide_strips_active" (read-only): some launch of the last run had wide strips
 *   "fuse"           time steps per HBM pass: -1 auto (the cheapest split of a run into passes of 2..7 steps, e.g.
 *                    1000 = 166 x 6 + 4, 20 = 7 + 7 + 6), 0/1 off, 2..7 balanced passes of at most that depth
 *   "variant"        single-step kernel family: 0 auto, 1 dpp, 2 lds, 3 naive
 *   "rows_per_chunk" rows one wavefront marches per launch (0 auto), "prefetch" (single-step kernel)
 *   "xcd_swizzle"    0/1 XCD-aware block->tile map; "tail_split" 0/1 (default 1): launches of two or more rounds of
 *                    wavefronts end with the top eighth of the rows in half-height chunks, dispatched last
 *   "overlap"        exchange schedule of a multi-rank run (all bit-identical): 0 serial exchange; 1 frame launch
 *                    first, the NEXT pass's exchange under the bulk launch; 3 frame and bulk in ONE launch: the frame wavefronts publish a flag the comm
 *                    stream waits on (hipStreamWaitValue64), so the exchange starts under the running kernel
 *                    without an event or a second launch (without signal memory: as 1); 4 bulk launch first with
 *                    THIS pass's exchange under it, then the frame launch — no pass of a run, not even the first,
 *                    waits for an unhidden exchange, and only stream order and events are involved; 5 (default) = 4
 *   "relay"          0/1 (default 1), schedule 4: the two streams swap roles every pass, so that the frame launch follows
 *                    the exchange chain, and the next pass's bulk launch the frame launch, on the same stream (no event
 *                    hand-off on the way of the data); "relay_events" 0/1 (default 0, experiment): the relay's cross-stream
 *                    events without the system-scope fence of a default event (+1 % on 20-step calls of the 8-GPU tile;
 *                    left off: what it skips is also what makes the field visible to other agents)
 *   "direct_faces"   0/1 (default 1), schedule 3: the frame wavefronts copy the cells that form the NEXT pass's faces
 *                    straight into the RCCL send buffers before they publish the flag (0: a pack kernel on the
 *                    comm stream does it after the flag)
 *   "frame_rows"     experiment: chunk height of the frame's side strips in a multi-rank pass (0 = default, the 12-14
 *                    rows of the bottom/top bands; measured best)
 *   "external_halo"  0/1 the caller carries the faces (csim_stepper_halo_* / _faces_*)
 *   "sync_timeout_ms" 0 (default): csim_stepper_sync waits as long as it takes; > 0: gives up with CSIM_ERR_TIMEOUT
 *   "test_stall"     test hook: 1 parks the comm stream on a signal value nobody publishes (what a lost flag or a
 *                    dead peer looks like from the host), 0 releases it
 *   "profile"        0 off, k >= 1: HIP events around the sweep launch(es) of every k-th pass
 *                    (csim_stepper_kernel_time)
 *   "autotune"       0/1 (default 1) with rows_per_chunk = 0: the first long run times the candidate
 *                    chunk heights on this GPU (trial launches that do not advance the field) and keeps
 *                    the fastest; "tuned_rows" (read-only) reports it, "last_rows" (read-only) the chunk
 *                    height the most recent fused launch actually used
 *   "last_regions", "last_tiles", "last_tail_blocks" (read-only): the tile plan of the most recent whole-field launch
 *                    of a fused pass — its regions (at most 8: left, wide and right strips of the main part and of the
 *                    half-height tail, and the two bands), its tiles, and the blocks dispatched last in plain order */
int csim_stepper_set_option(csim_stepper* s, const char* key, long value);
int csim_stepper_get_option(const csim_stepper* s, const char* key, long* value);
/* with option "profile"=1: HIP-event time and count of the sweep launches since the last reset, per kernel
 * kind: steps_per_launch = 1 selects the single-step kernel, 2..7 the kernels that advance that many time steps
 * per HBM pass (a multi-rank pass is one bracket around its frame and bulk launches; a single-rank run of equal
 * launches is one bracket, counted per launch).  The timer calls may follow csim_stepper_run directly: they wait
 * for every stream of the stepper the way csim_stepper_sync does (CSIM_ERR_RCCL / CSIM_ERR_TIMEOUT included,
 * after which the recorded events are kept for the next call) before they read the events */
int csim_stepper_kernel_time(csim_stepper* s, int steps_per_launch, double* total_ms,
                             long* launches);
/* same sampling, multi-rank runs over RCCL with "overlap" = 1: HIP-event time of the comm-stream chain
 * of a pass — packing the next pass's faces, the grouped ncclSend/ncclRecv exchange, unpack and ghost
 * fill — i.e. what the bulk sweep has to hide (replaces the blocking MPI_Waitall of reference
 * src/halo.cpp:46) */
int csim_stepper_comm_time(csim_stepper* s, double* total_ms, long* passes);
int csim_stepper_reset_timers(csim_stepper* s);

/* ---- ensemble: many small fields on one GPU ------------------------------------------------ */
/* B members share grid shape, spacing, boundary types and boundary value; each has its own field and its own
 * (D, dt, vx, vy).  A run advances every member exactly as csim_stepper_run advances a single-rank stepper holding
 * that member's field with its parameters (bit for bit, ghost ring included), with a few launches per pass for the
 * whole batch.  Host arrays use the reference layout per member; the _all variants take members x (ny+2) x (nx+2)
 * contiguous doubles.  One handle per GPU, not thread-safe.  Multi-rank members, per-member boundary types and the
 * "contract" mode are not supported. */
typedef struct csim_ensemble csim_ensemble;
int csim_ensemble_create(int members, int nx, int ny, int halo, double dx, double dy, const int bc[4],
                         double bc_value, csim_ensemble** out); /* zero-filled fields */
int csim_ensemble_destroy(csim_ensemble* e);
int csim_ensemble_upload(csim_ensemble* e, int member, const double* host_with_ghosts);
int csim_ensemble_download(csim_ensemble* e, int member, double* host_with_ghosts);
int csim_ensemble_upload_all(csim_ensemble* e, const double* host);
int csim_ensemble_download_all(csim_ensemble* e, double* host);
/* gaussian hotspot of one member, on the device, as csim_stepper_init_gaussian on one rank: the member's whole array,
 * ghost ring included, is zeroed first, in both ping-pong buffers */
int csim_ensemble_init_gaussian(csim_ensemble* e, int member, double A, double sigma_frac, double xc_frac,
                                double yc_frac);
/* one value per member each; dt is used as given (clamp with csim_safe_dt), it must be finite */
int csim_ensemble_set_physics(csim_ensemble* e, const double* D, const double* dt, const double* vx, const double* vy);
/* nsteps reference steps of every member, enqueued without host syncs: csim_ensemble_plan's passes */
int csim_ensemble_run(csim_ensemble* e, int nsteps);
int csim_ensemble_sync(csim_ensemble* e);
/* per member, each in one launch for the whole batch: csim_stepper_checksum's value of a one-rank stepper holding the
 * member's field (out[B]); min and max over the whole array, ghosts included (out[2B]: min, max of member 0, ...); the
 * sum over the interior (out[B]: per-block partial sums added in a fixed order, so the same field gives the same bits
 * every time; it may differ from another summation order in the last bits) */
int csim_ensemble_checksum(csim_ensemble* e, unsigned long long* out);
int csim_ensemble_minmax(csim_ensemble* e, double* out);
int csim_ensemble_sum(csim_ensemble* e, double* out);
/* per-cell statistics over the members, one launch for the whole batch: mean, variance (divided by members - ddof,
 * ddof 0 or 1, members - ddof >= 1), min and max, each in the reference layout (ny+2) x (nx+2), ghost ring included.
 * Bit for bit: s = +0, s += x_k in member order, mean = s / B; q = +0, q += (x_k - mean)^2 in member order,
 * var = q / (B - ddof); fmin / fmax in member order (NaN members skipped unless all are NaN) -- numpy's mean, var,
 * fmin.reduce and fmax.reduce over axis 0.  Any output may be NULL (not copied); synchronous.  No set_physics needed. */
int csim_ensemble_stats(csim_ensemble* e, int ddof, double* mean, double* var, double* min, double* max);
/* the same, captured without stalling: computed on the ensemble's stream after everything enqueued so far, copied to
 * pinned host buffers on a second stream; csim_ensemble_run may be called meanwhile.  A _begin while one is in flight
 * first waits for it. */
int csim_ensemble_stats_begin(csim_ensemble* e, int ddof);
/* pointers stay valid until the next _begin or destroy (any may be NULL); CSIM_ERR_STATE when nothing is in flight */
int csim_ensemble_stats_wait(csim_ensemble* e, const double** mean, const double** var, const double** min,
                             const double** max);
/* per-cell quantiles and exceedance probabilities over the members, one launch for the whole batch, each output field
 * in the reference layout (ny+2) x (nx+2), ghost ring included.  q[0..nq): levels in [0, 1] (numpy "linear");
 * thr[0..nt): out_p = (members with x > thr) / members.  out_q: nq fields, out_p: nt fields, one after the other;
 * either may be NULL (not copied).  0 <= nq, nt <= 16, nq + nt >= 1.  Synchronous.  No set_physics needed.
 * Bit for bit, per cell with s the members in ascending order and (lo, hi, g) = csim_ensemble_quantile_plan:
 * d = s[hi] - s[lo], g >= 0.5 ? s[hi] - d * (1 - g) : s[lo] + d * g, NaN if any member is NaN -- np.quantile(x, q,
 * axis=0) but for the sign of a zero result; out_p is np.mean(x > thr, axis=0).
 * At most 4096 members (csim_ensemble_create allows 65535): more give CSIM_ERR_UNSUPPORTED. */
int csim_ensemble_quantiles(csim_ensemble* e, int nq, const double* q, int nt, const double* thr,
                            double* out_q, double* out_p);
/* the same, captured as csim_ensemble_stats_begin captures (the kernel in stream order, the copy to pinned host
 * buffers on a stream of its own); a _begin while one is in flight first waits for it.  Statistics and quantiles may
 * be in flight together, and neither waits for the other's copy. */
int csim_ensemble_quantiles_begin(csim_ensemble* e, int nq, const double* q, int nt, const double* thr);
/* nq and nt fields of the capture; pointers stay valid until the next _begin or destroy (either may be NULL);
 * CSIM_ERR_STATE when nothing is in flight */
int csim_ensemble_quantiles_wait(csim_ensemble* e, const double** out_q, const double** out_p);
/* host-only: numpy's (lo, hi, gamma) of each level for this many members (v = (members - 1) * q; past the last index
 * lo = hi = members - 1 and gamma = v + 1, numpy's index -1) */
int csim_ensemble_quantile_plan(int members, int nq, const double* q, int* lo, int* hi, double* gamma);
/* verification of the members against one truth per cell, one launch for the whole batch.  The truth is either a
 * host field (truth, reference layout, copied before the call returns; truth_member = -1) and the M = B members are the
 * forecast, or member t = truth_member (truth = NULL) and the M = B - 1 others, in their order, are the forecast.
 * A cell is NaN when the truth or any forecast member is.  Per cell, without FMA contraction, every sum from +0:
 *   a = sum |x_k - y|;  lt = #(x_k < y), eq = #(x_k == y);  m = sum x_k / M;  v = sum (x_k - m)(x_k - m) / (M - 1)
 *   c = sum_{i=1}^{M-1} w_i (s_i - s_{i-1}), s the members ascending, w_i = (double)(i (M - i));
 *   CRPS = a / M - c / W, W = M M (fair = 0) or M (M - 1) (fair = 1, M >= 2);  NaN on a NaN cell
 *   Brier_k = (p - o)(p - o), p = #(x > thr_k) / M (as csim_ensemble_quantiles), o = y > thr_k ? 1 : 0;  NaN on a NaN
 *   cell.  out_crps: one field, out_brier: nt fields (0 <= nt <= CSIM_VERIFY_MAX_THRESHOLDS), ghost ring included.
 * Order of the sums a, sum x_k, sum (x_k - m)^2 (member order k) and c (sorted order i):
 *   M <= 64: one running sum in that order.
 *   M > 64: term k goes to lane k % 64; lane l sums its terms in increasing k from +0 (a lane without terms holds +0);
 *   the 64 lane sums are combined as l[j] = l[j] + l[j ^ h] for h = 32, 16, 8, 4, 2, 1, all j at once; the sum is l[0].
 * rank_hist (M + 1 bins) counts the non-NaN interior cells (i = 1..nx, j = 1..ny) at rank lt + mix(g) mod (eq + 1),
 * g = (j - 1) nx + (i - 1), mix the splitmix64 finaliser (csim_ensemble_rank_slot).  scores: over the n non-NaN
 * interior cells, the means of CRPS and of each Brier score, rmse = sqrt(sum (m - y)^2 / n), spread = sqrt(sum v / n)
 * (NaN when n = 0), from per-workgroup partial sums added in a fixed order: the same state gives the same bits.
 * Any output may be NULL (not computed on the host / not copied).  Synchronous.  No set_physics needed; the members'
 * fields are not modified.  Errors: CSIM_ERR_ARG unless exactly one truth is given, for truth_member outside -1 .. B-1,
 * nt outside 0 .. 16, fair not 0 / 1, fair with M < 2, no forecast member; CSIM_ERR_UNSUPPORTED for M > 4096. */
#define CSIM_VERIFY_MAX_THRESHOLDS 16
typedef struct csim_verify_scores {
    long long cells, nan_cells;
    double crps, rmse, spread;
    double brier[CSIM_VERIFY_MAX_THRESHOLDS]; /* first nt used, the rest 0 */
} csim_verify_scores;
int csim_ensemble_verify(csim_ensemble* e, const double* truth, int truth_member, int fair, int nt, const double* thr,
                         double* out_crps, double* out_brier, unsigned long long* rank_hist,
                         csim_verify_scores* scores);
/* the same, captured as csim_ensemble_quantiles_begin captures (kernel in stream order, the copy to pinned host buffers
 * on a stream of its own; a host truth is copied before the call returns).  A _begin while one is in flight first
 * waits for it.  Statistics, quantiles and verification may be in flight together. */
int csim_ensemble_verify_begin(csim_ensemble* e, const double* truth, int truth_member, int fair, int nt,
                               const double* thr);
/* the capture's fields and histogram (pointers valid until the next _begin or destroy; any may be NULL) and its scores,
 * finished here; CSIM_ERR_STATE when nothing is in flight */
int csim_ensemble_verify_wait(csim_ensemble* e, const double** out_crps, const double** out_brier,
                              const unsigned long long** rank_hist, csim_verify_scores* scores);
/* host-only: the rank histogram's tie-break, mix(g) mod (ties + 1) for g >= 0, ties >= 0 */
int csim_ensemble_rank_slot(long long g, int ties, int* slot);
/* neighbourhood and probability verification: the contingency table of the ensemble probability against the truth, and
 * the sums behind the Fractions Skill Score (Roberts & Lean 2008) over square neighbourhoods.  Forecast members and
 * truth as in csim_ensemble_verify: a host field (truth, truth_member = -1, M = B) or member t = truth_member
 * (truth = NULL, the M = B - 1 others, in their order, are the forecast).  Only interior cells take part (1 <= i <= nx,
 * 1 <= j <= ny); the ghost ring is never read as data.  A cell is NaN when its truth or any forecast member is NaN.
 * Per threshold thr[q] (1 <= nt <= CSIM_VERIFY_MAX_THRESHOLDS) and interior cell:
 *   n_q = #(x_k > thr[q]) over the forecast members (0 .. M);  o_q = y > thr[q] ? 1 : 0;  both 0 on a NaN cell.
 *   The comparisons are strict and IEEE: -0.0 > 0.0 is false, +Inf > thr unless thr is +Inf, nothing exceeds +Inf.
 * Everything the device computes is an integer, so the results do not depend on launch geometry or summation order:
 *   table[q][k][b]  (nt x (M + 1) x 2): the non-NaN interior cells with n_q == k and o_q == b;  cells / nan_cells: the
 *                   non-NaN / NaN interior cells.
 *   nbh[q][s][3]    (nt x ns x 3), scale s with half-width half[s], 0 <= ns <= CSIM_SPATIAL_MAX_SCALES,
 *                   0 <= half[s] <= CSIM_SPATIAL_MAX_HALF, any order, repeats allowed.  With w = 2 half[s] + 1, F(i, j)
 *                   is the sum of n_q over the w x w window centred on the cell and O(i, j) that of o_q; cells outside
 *                   the interior count as zero (zero padding, the usual convention of the score), and so do NaN cells.
 *                   Over the non-NaN interior centres: A = sum F F, Bo = sum O O, C = sum F O, in that order.
 *   counts          nt planes of ny x nx uint16_t holding n_q (no ghost ring);  flags: one uint32_t per interior cell,
 *                   bit q = o_q, bit 31 = NaN cell.
 * Any output may be NULL (not copied).  Synchronous.  No set_physics needed; no member's field is written.
 * Overflow: csim_verify_spatial_limit (host only) returns CSIM_ERR_UNSUPPORTED unless M <= CSIM_SPATIAL_MAX_MEMBERS and
 * M M w^4 nx ny <= 2^62, w = 2 half_max + 1.  Under that bound A <= 2^62, M M Bo <= 2^62 and 2 M C <= 2^63, so every
 * 64-bit unsigned sum below is exact, and a single F is below 2^32.  The compute entry points make the same check, with
 * the call's largest half-width (0 without scales), before anything is enqueued.  At M = 64 and half = 32 the bound
 * allows nx ny <= 63 073 416 (7941 x 7941; 8192 x 8192 up to half = 31); at M = 4096 and half = 32 only 15 398 cells
 * (124 x 124).
 * Errors: CSIM_ERR_ARG unless exactly one truth is given, for truth_member outside -1 .. B-1, nt outside 1 .. 16, ns
 * outside 0 .. 8, a half-width outside 0 .. 32, no forecast member; CSIM_ERR_UNSUPPORTED for M > 4096, the bound, or more than 2^27 interior cells. */
#define CSIM_SPATIAL_MAX_HALF 32
#define CSIM_SPATIAL_MAX_SCALES 8
#define CSIM_SPATIAL_MAX_MEMBERS 4096
int csim_ensemble_verify_spatial(csim_ensemble* e, const double* truth, int truth_member, int nt, const double* thr,
                                 int ns, const int* half, unsigned long long* table, unsigned long long* nbh,
                                 unsigned short* counts, unsigned int* flags, unsigned long long* cells,
                                 unsigned long long* nan_cells);
/* the same, captured as csim_ensemble_verify_begin captures (the kernels in stream order, the copy to pinned host
 * buffers on a stream of its own; a host truth is copied before the call returns), with a capture and a truth staging
 * of their own: statistics, quantiles, a plain verification and this one may all be in flight together, and
 * csim_ensemble_run may follow.  fields = 1: counts and flags are copied too; 0: only the tables.  A _begin while one
 * is in flight first waits for it. */
int csim_ensemble_verify_spatial_begin(csim_ensemble* e, const double* truth, int truth_member, int nt,
                                       const double* thr, int ns, const int* half, int fields);
/* the capture's outputs (pointers valid until the next _begin or destroy; any may be NULL; counts and flags are NULL
 * after a _begin with fields = 0); CSIM_ERR_STATE when nothing is in flight */
int csim_ensemble_verify_spatial_wait(csim_ensemble* e, const unsigned long long** table,
                                      const unsigned long long** nbh, const unsigned short** counts,
                                      const unsigned int** flags, unsigned long long* cells,
                                      unsigned long long* nan_cells);
/* host-only: the overflow bound above; CSIM_ERR_ARG for M, nx or ny < 1 or half_max outside 0 .. 32 */
int csim_verify_spatial_limit(int M, int nx, int ny, int half_max);
/* host-only: the scores of the tables, so that C, C++ and Python derive the same bits.  Per threshold, with T = table[q],
 * n = cells, p_k = (double)k / (double)M, every sum from +0 in increasing k, one rounding per operation, no contraction;
 * integer sums are exact and converted to double once:
 *   N_k = T[k][0] + T[k][1], O_k = T[k][1], SO = sum O_k, obar = (double)SO / (double)n
 *   brier       = (sum_k (p_k p_k (double)T[k][0] + (p_k - 1)(p_k - 1) (double)T[k][1])) / n
 *   reliability = (sum_{N_k > 0} (double)N_k (d d)) / n, d = p_k - f_k, f_k = (double)O_k / (double)N_k
 *   resolution  = (sum_{N_k > 0} (double)N_k (d d)) / n, d = f_k - obar
 *   uncertainty = obar (1 - obar);  brier = reliability - resolution + uncertainty up to rounding
 *   ROC: for the decision "at least k members exceed", hit_rate[q][k] = (double)(sum_{k' >= k} O_k') / (double)SO and
 *   false_alarm[q][k] = (double)(sum_{k' >= k} T[k'][0]) / (double)(n - SO), k = 0 .. M (both are 0 at k = M + 1);
 *   roc_area = sum over k = M down to 0 of ((F_k - F_{k+1}) (H_k + H_{k+1})) 0.5.  With SO = 0 the hit rates, with
 *   SO = n the false-alarm rates, and in both cases roc_area, are NaN.  With n = 0 every score of the threshold is NaN.
 *   fss[q][s]: in 64-bit unsigned integers S = A + M M Bo and D = S - 2 M C, which is sum (F - M O)^2 exactly;
 *   fss = 1 - (double)D / (double)S, NaN when S = 0.
 * hit_rate and false_alarm are the caller's: nt (M + 1) doubles each, or NULL.  Entries of `out` past nt / ns are 0.
 * CSIM_ERR_ARG for M < 1, nt outside 1 .. 16, ns outside 0 .. 8 or a null table / out (nbh may be NULL with ns = 0). */
typedef struct csim_spatial_scores {
    long long cells, nan_cells;
    double brier[CSIM_VERIFY_MAX_THRESHOLDS], reliability[CSIM_VERIFY_MAX_THRESHOLDS];
    double resolution[CSIM_VERIFY_MAX_THRESHOLDS], uncertainty[CSIM_VERIFY_MAX_THRESHOLDS];
    double roc_area[CSIM_VERIFY_MAX_THRESHOLDS];
    double fss[CSIM_VERIFY_MAX_THRESHOLDS][CSIM_SPATIAL_MAX_SCALES];
} csim_spatial_scores;
int csim_verify_spatial_finish(int M, int nt, int ns, const unsigned long long* table, const unsigned long long* nbh,
                               unsigned long long cells, unsigned long long nan_cells, csim_spatial_scores* out,
                               double* hit_rate, double* false_alarm);
/* analysis: pulls the forecast members towards point observations with the serial ensemble square-root filter
 * (Whitaker & Hamill 2002), localised with Gaspari & Cohn (1999).  Deterministic: no perturbed observations, no
 * random numbers, no matrix solves (every observation is a rank-1 update).
 * Observation o (0 <= o < nobs) is the interior cell (i[o], j[o]) of the reference layout (1 <= i <= nx,
 * 1 <= j <= ny, field [j, i]) with value y[o] and error variance r[o] > 0; the observation operator picks that cell.
 * The forecast members x_k, k = 0 .. M-1, are all B members (truth_member = -1), or the B - 1 others, in their order,
 * with truth_member = t (as csim_ensemble_verify); member t is not modified.  2 <= M <= CSIM_ASSIM_MAX_MEMBERS.
 * Localisation: rho = the table of csim_ensemble_gc_table(dx, dy, loc, nx, ny), with its half-widths lx, ly.
 * Inflation lambda >= 1: when lambda != 1, before the first observation every interior cell of every forecast member
 * becomes  x_k + (lambda - 1) (x_k - xbar),  xbar = sum x_k / M  (lambda - 1 formed on the host); lambda == 1 changes
 * nothing.  The observations are then taken one at a time, sorted by (level, input index), level from
 * csim_ensemble_assim_plan(nobs, i, j, lx, ly, ordered).  Per observation, without FMA contraction, every sum a
 * running sum from +0 in member order k = 0 .. M-1:
 *
 *     h_k = x_k(i_o, j_o);  hbar = sum h_k / M;  h'_k = h_k - hbar
 *     p = sum h'_k h'_k / (M-1);  d = p + r_o;  alpha = 1 / (1 + sqrt(r_o / d));  delta = y_o - hbar
 *     for every interior cell c = (i_o+a, j_o+b), |a| <= lx, |b| <= ly, with rho = rho[b+ly][a+lx] > 0:
 *         xbar = sum x_k(c) / M;  x'_k = x_k(c) - xbar
 *         cov  = sum x'_k h'_k / (M-1)
 *         g    = (rho cov) / d;  beta = alpha g
 *         x_k(c) <- x_k(c) + (g delta - beta h'_k)
 *
 * The division and the square root are IEEE fp64, correctly rounded.  Observations of one level are in disjoint
 * windows, so they commute exactly: the result is the serial filter in that order, whatever the launches.  The ghost
 * ring of every member (both ping-pong buffers), every cell outside all windows, and member t are left as they were.
 * Diagnostics, nobs values each in input order, any may be NULL: prior_mean, prior_var = hbar and p of each
 * observation at its turn; post_mean, post_var = sum x_k / M and sum (x_k - m)(x_k - m) / (M-1) at each observation's
 * cell after all observations.  *nlevels (may be NULL): the plan's level count.
 * With all four diagnostics NULL the call only enqueues its work on the ensemble's stream (the observations are copied
 * before it returns) and returns without waiting; otherwise it synchronises.  Statistics, quantile and verification
 * captures begun before the call see the state before the analysis.  No set_physics needed.  nobs = 0 with
 * lambda = 1 changes nothing.
 * Errors: CSIM_ERR_ARG for an observation outside the interior, r <= 0 or non-finite, y non-finite, loc <= 0 or
 * non-finite, lambda < 1 or non-finite, truth_member outside -1 .. B-1, M < 2, ordered not 0 / 1, nobs < 0, a null
 * i / j / y / r with nobs > 0; CSIM_ERR_UNSUPPORTED for M > CSIM_ASSIM_MAX_MEMBERS or nobs > CSIM_ASSIM_MAX_OBS. */
#define CSIM_ASSIM_MAX_MEMBERS 1024
#define CSIM_ASSIM_MAX_OBS (1 << 20)
int csim_ensemble_assimilate(csim_ensemble* e, int nobs, const int* i, const int* j, const double* y, const double* r,
                             double loc, double inflation, int truth_member, int ordered, double* prior_mean,
                             double* prior_var, double* post_mean, double* post_var, int* nlevels);
/* host-only: the Gaspari-Cohn localisation table.  loc = c > 0 in the units of dx and dy (support 2c).
 * lx = min(largest a >= 0 with (double)a * dx < 2 c, nx - 1), ly the same with dy and ny.  table (may be NULL: only
 * the sizes) gets (2 ly + 1) x (2 lx + 1) values, row b + ly, column a + lx:  GC(z), z = sqrt((a dx)^2 + (b dy)^2) / c,
 * each product and sum rounded in that order, and in Horner form
 *   z <= 1:     ((((-0.25 z + 0.5) z + 0.625) z - 5/3) z) z + 1
 *   1 < z < 2:  ((((z/12 - 0.5) z + 0.625) z + 5/3) z - 5) z + 4 - 2/(3 z)
 *   z >= 2:     0
 * (5/3 the rounded quotient, z/12 = z / 12, 2/(3 z) = 2 / (3 z), left to right: (... + 4) - 2/(3 z)), then
 * max(., +0).  The device only reads this table.  Errors: CSIM_ERR_ARG for dx, dy, loc
 * not finite and > 0, nx or ny < 1, null lx / ly. */
int csim_ensemble_gc_table(double dx, double dy, double loc, int nx, int ny, int* lx, int* ly, double* table);
/* host-only: the levels of csim_ensemble_assimilate.  Observations o and p conflict when |i_o - i_p| <= 2 lx and
 * |j_o - j_p| <= 2 ly (their windows may overlap).  ordered = 0 (first fit): in input order, each observation goes to
 * the lowest level holding no observation it conflicts with.  ordered = 1 (the caller's order kept): level(o) = 1 + the
 * highest level of an earlier observation conflicting with o, 0 when there is none.  level: nobs values;
 * *nlevels = 1 + the highest level (0 for nobs = 0).  Errors: CSIM_ERR_ARG for nobs < 0, lx or ly < 0, ordered not
 * 0 / 1, null arrays with nobs > 0, null nlevels; CSIM_ERR_UNSUPPORTED for nobs > CSIM_ASSIM_MAX_OBS. */
int csim_ensemble_assim_plan(int nobs, const int* i, const int* j, int lx, int ly, int ordered, int* level,
                             int* nlevels);
/* perturbation: adds sigma p_k to every interior cell of every forecast member k, p_k a unit-variance Gaussian random
 * field with the compact Gaspari-Cohn-shaped correlation of length corr_len, a pure function of (seed, draw, member
 * index, cell): additive inflation / model-error noise between analysis and forecast, or the spread of a fresh
 * ensemble, without a host round trip.  All fp64 arithmetic IEEE, without FMA contraction, every sum a running sum
 * from +0 in the stated order; integer arithmetic modulo 2^32 / 2^64.
 *
 * 1. Generator: Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9,
 *    0xBB67AE85, ten rounds), csim_philox4x32(ctr, key, out).
 * 2. Normal deviate from 64 bits, csim_normal_from_bits(bits, &z):  k = bits >> 12;  u = ((double)k + 0.5) 2^-52
 *    (exact, in (0, 1));  q = u - 0.5 (exact);  z = PPND16(u), Wichura's AS241 with its published coefficients, every
 *    polynomial of degree 7 in Horner form from the highest coefficient:
 *      |q| <= 0.425:  r = 0.180625 - q q;  z = (q A(r)) / B(r)
 *      otherwise:     t = q < 0 ? u : 1 - u;  r = sqrt(-ln t);  r <= 5: C(r - 1.6) / D(r - 1.6), else
 *                     E(r - 5) / F(r - 5);  negated for q < 0
 *    with the library's own ln:  (m, e) = frexp(t);  if m < the double nearest sqrt(1/2): m <- 2 m, e <- e - 1;
 *    s = (m - 1) / (m + 1);  w = s s;  p = 1/23;  for n = 21, 19, .., 1: p = p w + 1/n (1/n the rounded quotient);
 *    ln t = (double)e LN2 + 2 (s p),  LN2 = 0x3FE62E42FEFA39EF.  |z| <= 8.21.
 * 3. Taps along one axis, csim_ensemble_perturb_taps(d, corr_len, n, periodic, &R, taps), c = corr_len >= 0 in the
 *    units of dx, dy.  c == 0: R = 0, taps = {1}.  Otherwise R = min(largest a >= 0 with (double)a d < 2 c,
 *    periodic ? (n - 1) / 2 : n - 1);  g[o] = GC(((double)|o| d) / c), o = -R .. R, GC the Horner forms of
 *    csim_ensemble_gc_table, then max(., +0);  S = sum g[o] g[o] in increasing o;  taps[o + R] = g[o] / sqrt(S).
 *    The device only reads the two tables tx (dx, nx) and ty (dy, ny), of radii Rx and Ry.
 * 4. Lattice.  Axis x is periodic iff bc[LEFT] == bc[RIGHT] == PERIODIC, y likewise with BOTTOM / TOP.  The noise
 *    lives on Px x Py lattice points, Px = nx on a periodic axis, else nx + 2 Rx.  Interior column i = 1 .. nx with
 *    offset o reads lattice column a(i, o) = (i - 1 + o) mod nx (periodic) or i - 1 + o + Rx; rows b(j, o) the same.
 *    L = b Px + a as a 64-bit integer.  A periodic field gets seamless noise, a bounded one unit variance up to its
 *    edge.
 * 5. White noise.  w_k(L) = normal_from_bits(out[2 s] | out[2 s + 1] << 32), s = L & 1,
 *    out = philox(ctr = (lo32(L >> 1), hi32(L >> 1), k, draw), key = (lo32(seed), hi32(seed))).  k is the member's
 *    index in the ensemble (not its position among the forecast members): member k's field depends neither on B nor
 *    on truth_member.
 * 6. Smoothing, x first:  hx_k(b, i) = sum_{o = -Rx .. Rx} tx[o] w_k(b Px + a(i, o)), then
 *    p_k(i, j) = sum_{o = -Ry .. Ry} ty[o] hx_k(b(j, o), i),  each product rounded, sums in increasing o.
 * 7. Centring and update.  The forecast members are all B (truth_member = -1) or the B - 1 others (member t is not
 *    modified), as in csim_ensemble_verify; M of them.  centered = 1: pbar(i, j) = (sum_k p_k) / M in member order,
 *    p_k <- p_k - pbar, so that the ensemble mean moves by rounding only; the fields are NOT rescaled by
 *    sqrt(M / (M - 1)), their variance is (M - 1) / M.  Then x_k <- x_k + sigma p_k on every interior cell.
 * The ghost ring of every member (both ping-pong buffers), the buffer that is not current and member t are left as
 * they were.  sigma == 0 changes nothing and launches nothing.  The call enqueues on the ensemble's stream and returns
 * without waiting, so run -> perturb -> run and assimilate -> perturb -> run need no host round trip; statistics,
 * quantile and verification captures begun before the call see the state before it.  No set_physics needed.
 * Errors: CSIM_ERR_ARG for sigma or corr_len not finite, corr_len < 0, centered not 0 / 1, truth_member outside
 * -1 .. B-1, no forecast member, centered with M < 2; CSIM_ERR_UNSUPPORTED for Rx or Ry > CSIM_PERTURB_MAX_RADIUS. */
#define CSIM_PERTURB_MAX_RADIUS 32
int csim_ensemble_perturb(csim_ensemble* e, unsigned long long seed, unsigned draw, double sigma, double corr_len,
                          int centered, int truth_member);
/* host-only: item 1.  Known answers: ctr 0 0 0 0, key 0 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8 */
int csim_philox4x32(const unsigned ctr[4], const unsigned key[2], unsigned out[4]);
/* host-only: item 2 */
int csim_normal_from_bits(unsigned long long bits, double* z);
/* host-only: item 3; taps (may be NULL: only *R) gets 2 R + 1 values.  Errors: CSIM_ERR_ARG for d not finite and > 0,
 * corr_len not finite and >= 0, n < 1, periodic not 0 / 1, null R; CSIM_ERR_UNSUPPORTED for
 * R > CSIM_PERTURB_MAX_RADIUS */
int csim_ensemble_perturb_taps(double d, double corr_len, int n, int periodic, int* R, double* taps);
/* relaxation inflation: after an analysis, pulls the analysis perturbations of every interior cell back towards the
 * forecast ones, cell by cell: relaxation to prior spread (RTPS, Whitaker & Hamill 2012) or to prior perturbations
 * (RTPP, Zhang et al. 2004).  Unlike the multiplicative inflation of csim_ensemble_assimilate and the additive noise
 * of csim_ensemble_perturb it is selective in space: where no observation acted nothing changes, where the analysis
 * removed spread part of it is given back.  The cycle is  run -> prior_capture -> assimilate -> relax -> run.
 * The forecast members x_k, k = 0 .. M-1, are all B members (truth_member = -1) or the B - 1 others in their order
 * (member t is never read or written), as in csim_ensemble_assimilate; 2 <= M <= CSIM_ASSIM_MAX_MEMBERS.  Interior
 * cells only (i = 1 .. nx, j = 1 .. ny).  All fp64 arithmetic IEEE, without FMA contraction, / and sqrt correctly
 * rounded, every sum a running sum from +0 in member order k = 0 .. M-1.  Per cell:
 *
 *     mv(x):  s = sum x_k;  m = s / M;  q = sum (x_k - m)(x_k - m);  v = q / (M-1)
 *
 * capture, CSIM_RELAX_SPREAD:  (m_b, v_b) = mv(x);  sb = sqrt(v_b) is kept in a device field of the handle.
 * capture, CSIM_RELAX_PERT:    every member is kept as it is, xb_k, in a device copy of the handle (the size of one
 *     ping-pong buffer, allocated at the first such capture and kept until destroy).
 * relax, CSIM_RELAX_SPREAD:    (m, v) = mv(x);  sa = sqrt(v);  f = sa > 0 ? alpha ((sb - sa) / sa) : +0.
 *     Where f == 0 the cell is NOT written; elsewhere  x_k <- x_k + f (x_k - m)  for every forecast member.  (f < 0,
 *     where the analysis spread exceeds the prior's, deflates; a NaN sa gives f = +0, a NaN sb with sa > 0 gives NaN.)
 *     Outside every observation window an analysis leaves the members' bits alone, so sa is computed from the same
 *     bits in the same order as sb, sb - sa is exactly +0 and the cell keeps its bits, a -0 included.
 * relax, CSIM_RELAX_PERT:      m = mv(x).m;  m_b = mv(xb).m;  x_k <- x_k + alpha ((xb_k - m_b) - (x_k - m))  for every
 *     forecast member, every cell.
 *
 * alpha is finite, 0 <= alpha <= 1; alpha == 0 changes nothing and launches nothing (out_factor then gets +0
 * everywhere).  out_factor (RTPS only, may be NULL; must be NULL for RTPP): a host field in the reference layout,
 * (ny+2) x (nx+2), that gets f on the interior and +0 on the ghost ring.  With out_factor == NULL the call only enqueues
 * on the ensemble's stream and returns without waiting, so capture -> assimilate -> relax -> perturb -> run needs no
 * host round trip; with it the call synchronises.  Both calls are ordered on the ensemble's stream: statistics,
 * quantile and verification captures begun before relax see the state before it.  The ghost ring of every member
 * (both ping-pong buffers), the buffer that is not current and member t are left as they were.  No set_physics needed.
 * Validity: a capture is valid for relax with the same mode and the same truth_member until the next
 * csim_ensemble_run with nsteps > 0 (a guard against relaxing towards a stale forecast) or the next capture of either
 * mode.  relax consumes nothing: a second call relaxes the relaxed state against the same prior.  Assimilation,
 * perturbation, statistics, quantiles, verification, a run of 0 steps, uploads and init_gaussian do not invalidate a
 * capture (its storage is the handle's own, not a ping-pong buffer).
 * Errors: CSIM_ERR_ARG for mode not 1 / 2, truth_member outside -1 .. B-1, M < 2, alpha not finite or outside [0, 1],
 * out_factor with RTPP; CSIM_ERR_UNSUPPORTED for M > CSIM_ASSIM_MAX_MEMBERS; CSIM_ERR_STATE for relax without a valid
 * capture of that mode and truth member.  Errors are reported before anything is enqueued and leave the members and a
 * valid capture as they were. */
#define CSIM_RELAX_SPREAD 1 /* RTPS */
#define CSIM_RELAX_PERT 2   /* RTPP */
int csim_ensemble_prior_capture(csim_ensemble* e, int mode, int truth_member);
int csim_ensemble_relax(csim_ensemble* e, int mode, double alpha, int truth_member, double* out_factor);
/* observation network: the observations of an analysis as an object that lives on the device.  It is planned once
 * (cells, error variances, localisation, levels); its values are drawn on the GPU from a member, with seeded noise, or
 * set from the host; the analysis reads it without staging and logs innovation statistics on the device, to be fetched
 * once.  A K-cycle observing-system simulation experiment,
 *     run -> observe -> prior_capture -> assimilate_network(record) -> relax -> perturb,   K times, then one log,
 * is K enqueue-only cycles and one fetch.  All fp64 arithmetic IEEE, without FMA contraction, every product rounded.
 *
 * create: observation o (0 <= o < nobs, nobs >= 1) is the interior cell (i[o], j[o]) with error variance r[o], loc and
 *   ordered as in csim_ensemble_assimilate, and validated as there (CSIM_ERR_ARG: a cell outside the interior, r not
 *   finite and > 0, loc not finite and > 0, ordered not 0 / 1, nobs < 1, log_cycles outside 0 .. 65536, a null array;
 *   CSIM_ERR_UNSUPPORTED: nobs > CSIM_ASSIM_MAX_OBS).  The table and lx, ly are those of csim_ensemble_gc_table, the
 *   levels those of csim_ensemble_assim_plan, the order (level, input index).  Everything the kernels read is put on
 *   the device once, sqrt(r_o) (correctly rounded) included, with room for the values, the log of log_cycles records
 *   and the diagnostics.  The network is bound to the ensemble's geometry and stream; csim_ensemble_destroy destroys
 *   the networks that are still alive, and their handles are invalid from then on.
 * info: any pointer may be NULL.
 * set_values: y[o], nobs finite values in input order (a non-finite one: CSIM_ERR_ARG, before anything is enqueued),
 *   copied before the call returns; the call only enqueues.  Clears has_truth.
 * observe: for every o, xt_o = x_s(i_o, j_o), s = source_member, in the current buffer after everything enqueued so
 *   far.  noise = 1:  y_o = xt_o + sqrt(r_o) z_o  (the product rounded, then the sum);  noise = 0:  y_o = xt_o, its
 *   bits (a -0 stays).  z_o = the value of csim_obs_noise for (seed, draw, o):
 *   csim_normal_from_bits of  out[0] | out[1] << 32,  out = csim_philox4x32 with ctr = (o, 0, 0xFFFFFFFF, draw),
 *   key = (lo32(seed), hi32(seed)).  Counter word 2 is no member index, so the stream is disjoint from every field of
 *   csim_ensemble_perturb under the same seed and draw; z_o depends on the input index o alone.  xt is kept and
 *   has_truth set.  Only enqueues.  CSIM_ERR_ARG: source_member outside 0 .. B-1, noise not 0 / 1.
 * assimilate_network: the analysis of csim_ensemble_assimilate with (i, j, y, r, loc, ordered) of the network and the
 *   inflation and truth_member given, bit for bit, and always only enqueued: no host planning, no staging copy.
 *   record = 1 also computes, per observation at its cell, with mv of csim_ensemble_relax over the forecast members:
 *   (hb_o, vb_o) = mv(x) before the inflation and the first observation, (ha_o, va_o) = mv(x) after the last (the
 *   post_mean and post_var of csim_ensemble_assimilate), and appends one csim_obs_cycle to the log on the device.
 *   Every sum_ field: for each chunk c of 256 consecutive input indices T_c = the running sum of the terms from +0 in
 *   input order; the field = the running sum of T_c from +0 in chunk order.  Terms:
 *     n = (double)nobs;  has_truth = 0 or 1
 *     ob: y - hb;  ob2: (y - hb)(y - hb);  oa: y - ha;  oa2: (y - ha)(y - ha);  oa_ob: (y - ha)(y - hb)
 *     ab_ob: (ha - hb)(y - hb);  vb: vb;  va: va;  r: r
 *     eb2: (hb - xt)(hb - xt);  ea2: (ha - xt)(ha - xt);  both sums +0 when has_truth is 0
 *   (sum_oa_ob / sum_r is the ratio of Desroziers et al. 2005, 1 for consistent error statistics.)
 *   Errors, all before anything is enqueued: those of csim_ensemble_assimilate for inflation, truth_member and M;
 *   CSIM_ERR_ARG for a network of another ensemble and record not 0 / 1; CSIM_ERR_STATE when the network has no values
 *   yet, and with record = 1 when the log is full or log_cycles is 0.  Values stay valid until they are replaced.
 * fetch: synchronises the ensemble's stream; y, truth (= xt; CSIM_ERR_STATE when has_truth is 0) and bg_mean, bg_var,
 *   post_mean, post_var (hb, vb, ha, va of the last recorded analysis; CSIM_ERR_STATE when there is none), nobs values
 *   each in input order.  Any pointer may be NULL.
 * log: synchronises; out gets min(max, cycles) records, oldest first; *ncycles (may be NULL) the number recorded since
 *   create or the last reset.  log_reset is enqueued. */
typedef struct csim_obs_network csim_obs_network;
int csim_obs_network_create(csim_ensemble* e, int nobs, const int* i, const int* j, const double* r, double loc,
                            int ordered, int log_cycles, csim_obs_network** out);
int csim_obs_network_destroy(csim_obs_network* n);
int csim_obs_network_info(const csim_obs_network* n, int* nobs, int* nlevels, int* lx, int* ly);
int csim_obs_network_set_values(csim_obs_network* n, const double* y);
int csim_obs_network_observe(csim_obs_network* n, int source_member, unsigned long long seed, unsigned draw,
                             int noise);
/* host-only: z_o of observe */
int csim_obs_noise(unsigned long long seed, unsigned draw, unsigned o, double* z);
int csim_ensemble_assimilate_network(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                     int record);
int csim_obs_network_fetch(csim_obs_network* n, double* y, double* truth, double* bg_mean, double* bg_var,
                           double* post_mean, double* post_var);
typedef struct csim_obs_cycle {
    double n, has_truth, sum_ob, sum_ob2, sum_oa, sum_oa2, sum_oa_ob, sum_ab_ob, sum_vb, sum_va, sum_r, sum_eb2,
        sum_ea2;
} csim_obs_cycle;
int csim_obs_network_log(csim_obs_network* n, int max, csim_obs_cycle* out, int* ncycles);
int csim_obs_network_log_reset(csim_obs_network* n);
/* linear observations: a network whose observations are linear functionals of the state, a station between grid
 * points (interpolated) or a footprint (an area average), instead of one cell each.  Observation o has an anchor
 * (i_o, j_o) in the interior, an error variance r_o and the taps s = start[o] .. start[o+1]-1, each (di_s, dj_s, w_s).
 * The anchor centres the localisation window and enters the level plan, exactly as the observed cell of a point
 * observation does; the taps define what is observed.  Operator value, without FMA contraction, every product rounded,
 * a running sum from +0 in tap order:
 *
 *     h_k = sum_s  w_s * x_k(i_o + di_s, j_o + dj_s)
 *
 * Everything after h_k is the text of csim_ensemble_assimilate: hbar = sum h_k / M;  h'_k = h_k - hbar;
 * p = sum h'_k h'_k / (M-1);  d = p + r_o;  alpha = 1 / (1 + sqrt(r_o / d));  delta = y_o - hbar;  the window update
 * for every interior cell c = (i_o+a, j_o+b), |a| <= lx, |b| <= ly, with rho > 0, centred on the anchor; the levels of
 * csim_ensemble_assim_plan on the anchors; plan order (level, input index).
 * Constraints, checked before anything is enqueued (CSIM_ERR_ARG): 1 <= taps per observation <= CSIM_OBS_MAX_TAPS;
 * start[0] == 0 and start non-decreasing; every tapped cell interior; every w_s finite; |di_s| <= lx and |dj_s| <= ly,
 * lx and ly those of csim_ensemble_gc_table.  The last constraint is what keeps the plan valid unchanged: two
 * observations of one level have anchors more than 2 lx apart along x or more than 2 ly apart along y, so a tap at
 * most lx / ly from its anchor lies outside every other window of that level, no observation of a level reads a cell
 * that another one of that level writes, and the observations of a level still commute exactly.  Repeated cells and
 * negative weights are allowed.  A one-tap observation (0, 0, 1.0) gives h_k = +0 + 1.0 x_k = x_k: the point
 * observation bit for bit, except that a -0 in the field becomes +0.
 * Diagnostics and the log follow the operator: observe gives xt_o = h of the source member (noise as before:
 * y_o = xt_o + sqrt(r_o) z_o, z_o = csim_obs_noise of the input index; noise = 0: y_o = xt_o); (hb, vb) and (ha, va)
 * are mv of csim_ensemble_relax applied to h_k over the forecast members, before the inflation and after the last
 * observation; csim_obs_cycle keeps its thirteen fields and their chunked sums.
 * create_linear: as csim_obs_network_create with (i, j) the anchors, plus start (nobs + 1 values), di, dj, w
 *   (start[nobs] values each); the constraints above are those of csim_obs_linear_check with the ensemble's nx, ny and
 *   the lx, ly of loc.  The result is a csim_obs_network: set_values, observe, csim_ensemble_assimilate_network, fetch,
 *   log, log_reset, info and destroy work on it unchanged.  An error leaves the ensemble and every existing network as
 *   they were.  CSIM_ERR_ARG also for a null start / di / dj / w.
 * taps: *ntaps_total = start[nobs] of a linear network, 0 of a point network.
 * linear_check (host-only, needs no device): CSIM_OK or CSIM_ERR_ARG with the first violated constraint in
 *   csim_last_error; also CSIM_ERR_ARG for nobs < 1, nx or ny < 1, lx or ly < 0, a null array, an anchor outside the
 *   interior.
 * taps_bilinear (host-only): the four taps of bilinear interpolation to (x, y) in cell-index units, 1 <= x <= nx,
 *   1 <= y <= ny (else CSIM_ERR_ARG).  *i = min(floor(x), nx - 1), and max(., 1) when nx == 1, where the x taps
 *   collapse onto the one column (di = 0 for all four); fx = x - *i; *j and fy the same from y and ny.  Taps in the
 *   order (0,0) (1,0) (0,1) (1,1) with weights (1-fx)(1-fy), fx (1-fy), (1-fx) fy, fx fy, each difference and product
 *   rounded in that order.
 * taps_box (host-only): the mean over the (2a+1) x (2b+1) box around the interior cell (i, j), a, b >= 0, clipped to
 *   the interior: rows in increasing dj, then increasing di; every weight 1 / count, the rounded quotient; *ntaps =
 *   count; di, dj, w have room for CSIM_OBS_MAX_TAPS.  CSIM_ERR_UNSUPPORTED above CSIM_OBS_MAX_TAPS taps,
 *   CSIM_ERR_ARG for (i, j) outside the interior, a or b < 0, a null pointer. */
#define CSIM_OBS_MAX_TAPS 64
int csim_obs_network_create_linear(csim_ensemble* e, int nobs, const int* i, const int* j, const int* start,
                                   const int* di, const int* dj, const double* w, const double* r, double loc,
                                   int ordered, int log_cycles, csim_obs_network** out);
int csim_obs_network_taps(const csim_obs_network* n, int* ntaps_total);
int csim_obs_linear_check(int nx, int ny, int lx, int ly, int nobs, const int* i, const int* j, const int* start,
                          const int* di, const int* dj, const double* w);
int csim_obs_taps_bilinear(int nx, int ny, double x, double y, int* i, int* j, int di[4], int dj[4], double w[4]);
int csim_obs_taps_box(int nx, int ny, int i, int j, int a, int b, int* ntaps, int* di, int* dj, double* w);
/* screening: which observations of a network an analysis uses, decided per cycle on the device without a host round
 * trip: a mask for reports that are missing, and a background (gross-error) check that rejects an observation whose
 * innovation is large against background variance + r.  Each observation has a status byte for the last analysis:
 * CSIM_OBS_USED 0, CSIM_OBS_INACTIVE 1, CSIM_OBS_REJECTED 2.  Point and linear networks alike.
 * set_active: active[o], nobs bytes in input order, each 0 or 1 (any other value: CSIM_ERR_ARG, before anything is
 *   enqueued); NULL: all active.  Copied before the call returns; the call only enqueues.  The mask belongs to the
 *   network and stays until it is replaced; a new network is all active.  Values, has_truth, the log and the
 *   diagnostics are not touched.
 * assimilate_screened: tol finite and >= 0; tol == 0: no background check, only the mask acts.
 *   1. (hb_o, vb_o) = mv of csim_ensemble_relax applied to h_k of the observation (point or linear) over the forecast
 *      members, before the inflation and the first observation: what record = 1 stores.
 *   2. k2 = tol * tol, the rounded product, formed on the host.  Per observation, without FMA contraction:
 *          t = y_o - hb_o;   lhs = t * t;   rhs = k2 * (vb_o + r_o)
 *   3. status_o = INACTIVE where the mask says so (the mask wins; y_o of an inactive observation is never looked at);
 *      else REJECTED iff tol > 0 and !(lhs <= rhs): a NaN rejects, equality keeps; else USED.
 *   4. The analysis of csim_ensemble_assimilate follows.  The inflation is applied as before to every interior cell,
 *      whatever the statuses; the serial filter runs over the USED observations only, in the plan order
 *      (level, input index) of the full network.  An observation that is not USED takes no turn: it reads nothing and
 *      writes nothing.  Observations of one level commute exactly, so a subset of a level still does, and the levels and
 *      launches of the full plan stay valid.
 *   Two consequences.  ordered = 1: the result is that of csim_ensemble_assimilate with just the USED observations, in
 *   input order, ordered = 1, bit for bit (conflicting pairs keep their input order in both plans, the others commute
 *   exactly).  ordered = 0: the order is that of the full plan; a first-fit plan of the subset may order a conflicting
 *   pair differently, so that identity is not claimed.
 *   csim_ensemble_assimilate_network(e, n, lambda, t, record) is this call with tol = 0.  With an all-active mask
 *   (never set, NULL, or all ones) and tol == 0 nothing is screened: no status is computed, the analysis launches what
 *   it launched before this block existed, and gives the same bits.
 *   record = 1: (hb, vb) and (ha, va) are stored for every observation, whatever its status.  Every sum_ field of
 *   csim_obs_cycle keeps its chunks of 256 consecutive input indices; the term of an observation that is not USED is
 *   +0, which leaves the bits of a running sum that started from +0: the sums over the USED observations.  n = the
 *   number of USED observations.  A second log runs parallel to the first: per recorded cycle one
 *   csim_obs_screen_cycle, the counts n_used (== n), n_inactive and n_rejected as doubles, with room for log_cycles
 *   records; log_reset resets both.  record = 0 with tol > 0 computes (hb, vb) into storage that fetch does not read: bg_* / post_* of
 *   fetch stay those of the last recorded analysis.
 *   Errors, all before anything is enqueued, leaving members, values, mask, log and diagnostics as they were: those of
 *   csim_ensemble_assimilate_network; CSIM_ERR_ARG for tol not finite or < 0.
 * screen_log: as log, for the csim_obs_screen_cycle records.
 * status: synchronises the ensemble's stream; nobs bytes in input order for the last analysis of this network, recorded
 *   or not.  CSIM_ERR_STATE before the first analysis; after an analysis that screened nothing every byte is 0.
 *   CSIM_ERR_ARG for a null pointer.
 * screen_decide (host-only, needs no device): *status of steps 2 and 3 for one observation; active is 0 or 1
 *   (CSIM_ERR_ARG otherwise, and for tol not finite or < 0, and a null status). */
#define CSIM_OBS_USED 0
#define CSIM_OBS_INACTIVE 1
#define CSIM_OBS_REJECTED 2
int csim_obs_network_set_active(csim_obs_network* n, const unsigned char* active);
int csim_ensemble_assimilate_screened(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                      int record, double tol);
typedef struct csim_obs_screen_cycle {
    double n_used, n_inactive, n_rejected;
} csim_obs_screen_cycle;
int csim_obs_network_screen_log(csim_obs_network* n, int max, csim_obs_screen_cycle* out, int* ncycles);
int csim_obs_network_status(csim_obs_network* n, unsigned char* status);
int csim_obs_screen_decide(double y, double hb, double vb, double r, double tol, int active, int* status);
/* forecast impact: which observations of a network helped the forecast, and by how much: ensemble forecast sensitivity
 * to observations (EFSOI; Kalnay et al. 2012, localised as in Hotta et al. 2017).  No adjoint, no data-denial runs.  With
 * d = y - hb the innovations of a recorded analysis, Ya the analysis perturbations in observation space, Xf the forecast
 * perturbations at verification time, M forecast members, e_a and e_b the errors of the mean forecasts from the analysis
 * and from the background, and C a norm,
 *
 *     e_a' C e_a - e_b' C e_b  ~=  1/(M-1)  d' R^-1 Ya [rho o Xf' C (e_a + e_b)]  =  sum_o J_o
 *
 * J_o is the impact of observation o; J_o < 0: it reduced the forecast error.  rho is the network's own table around
 * the observation's cell or anchor, where it was at analysis time (static localisation: rho is not advected with the
 * flow), and a multiplicative inflation, a relaxation or a perturbation between the analysis and the capture enters only
 * through the perturbations that are captured.  The cycle is
 *     assimilate_network(record) [-> relax -> perturb] -> impact_capture -> run -> obs_impact(weight),
 * the caller forming weight = C (e_a + e_b) on the host.  Point and linear networks alike.  All fp64 arithmetic IEEE,
 * without FMA contraction, every product rounded, / correctly rounded.
 * impact_capture: only enqueues.  The network's last analysis must be one recorded with record = 1; the M forecast
 *   members are all B (truth_member = -1) or the B - 1 others in their order, as in csim_ensemble_assimilate.  For every
 *   observation o, in the current buffer after everything enqueued so far:  h_k of forecast member k, the cell of a point
 *   observation (its bits), sum_s w_s x_k(anchor + tap s) of a linear one as in csim_obs_network_create_linear;
 *       ha = sum h_k / M  (a running sum from +0 in member order);   a_{o,k} = h_k - ha
 *   kept as M doubles per observation in storage of the network's own, made at the first capture and kept until destroy.
 *   Also kept:  dn_o = (y_o - hb_o) / r_o  from the network's values as they are now and the bg_mean of the recorded
 *   analysis (one subtraction, one division), and that analysis's status byte; every observation counts as USED when it
 *   was not screened.  Of an observation that is not USED only the byte is kept.  Later observe / set_values /
 *   set_active calls, later analyses of either kind, runs and uploads leave a capture as it is: it ends at the next
 *   capture or at destroy.
 *   Errors, all before anything is enqueued, leaving an earlier capture as it was: CSIM_ERR_ARG for truth_member outside
 *   -1 .. B-1 and M < 2; CSIM_ERR_UNSUPPORTED for M > CSIM_ASSIM_MAX_MEMBERS and for nobs M > CSIM_IMPACT_MAX_DOUBLES
 *   (1 GiB of perturbations); CSIM_ERR_STATE when the network's last analysis was not a recorded one (there is none, or
 *   an unrecorded one has replaced its status bytes since).
 * obs_impact: synchronous, as csim_ensemble_verify.  e is the network's ensemble at verification time; its forecast
 *   members are those of the capture (the same truth_member).  weight: a host field in the reference layout,
 *   (ny+2) x (nx+2); only the interior is read, every interior value must be finite; it is copied before any kernel
 *   runs.  Per USED observation o, with the table rho and half-widths lx, ly of the network, the window of the analysis
 *   clipped to the interior, i0 = max(1, i_o - lx) .. i1 = min(nx, i_o + lx), j0 .. j1 likewise, and its cells numbered
 *   row-major, e = (j - j0) (i1 - i0 + 1) + (i - i0), e = 0 .. cells-1:
 *
 *       cell e with rho = rho[j - j_o + ly][i - i_o + lx] > 0:
 *           xbar = sum x_k / M;   c = sum (x_k - xbar) a_{o,k}      (running sums from +0 in member order k = 0 .. M-1)
 *           u_e  = (rho (c / (M-1))) weight[j][i]
 *       cell e with rho == 0:   u_e = +0, whatever the cell holds
 *       S_o = fold(u_0 .. u_{cells-1});   J_o = dn_o S_o
 *
 *   fold is the lane rule of csim_ensemble_verify for M > 64, applied to cells (csim_obs_impact_fold): term e goes to
 *   lane e % 64; lane l sums its terms in increasing e from +0 (a lane without terms holds +0); the 64 lane sums are
 *   combined as l[j] = l[j] + l[j ^ h] for h = 32, 16, 8, 4, 2, 1, all j at once; the sum is l[0].  An observation that is
 *   not USED gets J_o = +0.  No result depends on the launch geometry.
 *   out_impact (may be NULL): nobs values in input order.  summary (may be NULL): used = the number of USED
 *   observations, beneficial = the number with J_o < 0, total = sum J_o in input order by the chunk rule of
 *   csim_obs_cycle: T_c over 256 consecutive input indices from +0, then the running sum of T_c from +0.
 *   Errors, leaving the capture and everything else as it was: CSIM_ERR_ARG for a null ensemble, network or weight, a
 *   network of another ensemble, a non-finite interior weight; CSIM_ERR_STATE without a capture.
 * Neither call writes a member, a ghost ring or the other ping-pong buffer, nor the network's values, mask, logs or
 * diagnostics.
 * impact_fold (host-only, needs no device): *S = fold(u_0 .. u_{n-1}); n == 0 gives +0.  CSIM_ERR_ARG for n < 0, a null
 *   S, a null u with n > 0.
 * obs_impact_global: the same estimate without localisation (rho = 1 over the whole domain; Kalnay et al. 2012 as
 *   written), for a global filter.  The capture, the weight, out_impact, summary with its chunk rule, the synchrony and
 *   the "writes nothing" clause are those of obs_impact.  Without rho the sum over the cells factors, and the members
 *   are read once, whatever the network:  M and truth_member are the capture's;
 *       g_k = csim_ensemble_dot(centered = 1, K = 1, weight)[k]        (k = 0 .. M-1)
 *   and per USED observation o, with the captured a_{o,k} and dn_o:
 *       c = +0;  c = c + a_{o,k} * g_k  (k = 0 .. M-1);   S_o = c / (M-1);   J_o = dn_o * S_o
 *   An observation that is not USED gets J_o = +0; nothing of its capture is read.
 *   Errors: those of obs_impact, in its order; then CSIM_ERR_UNSUPPORTED when the capture has more than
 *   CSIM_ESPACE_MAX_MEMBERS forecast members.
 *   What is claimed.  The call does not know which filter made the capture.  The estimate's premise is the gain
 *   K = Xa Ya' R^-1 / (M-1).  After csim_ensemble_assimilate_etkf and _etkf_device that holds exactly, whatever the
 *   inflation, and where the forecast is linear in the state (all members with one (D, dt, vx, vy), static sides) the
 *   total equals the actual change of the squared error of the mean forecast up to rounding.  After
 *   csim_ensemble_assimilate_letkf, _local and the serial filter the gain is localised: use obs_impact.
 * obs_impact_global_value (host-only, needs no device): the three operations above for one observation, M >= 2 values
 *   a and g; CSIM_ERR_ARG for M < 2 and a null pointer. */
#define CSIM_IMPACT_MAX_DOUBLES (1L << 27)
typedef struct csim_obs_impact_summary {
    long long used, beneficial;
    double total;
} csim_obs_impact_summary;
int csim_obs_network_impact_capture(csim_obs_network* n, int truth_member);
int csim_ensemble_obs_impact(csim_ensemble* e, csim_obs_network* n, const double* weight, double* out_impact,
                             csim_obs_impact_summary* summary);
int csim_obs_impact_fold(const double* u, long n, double* S);
int csim_ensemble_obs_impact_global(csim_ensemble* e, csim_obs_network* n, const double* weight, double* out_impact,
                                    csim_obs_impact_summary* summary);
int csim_obs_impact_global_value(int M, const double* a, const double* g, double dn, double* J);
/* local analysis: every interior cell is analysed on its own from all observations of a network near it, with the
 * localisation applied to the observation error (R-localisation; Hunt et al. 2007, the LETKF).  Cells are independent,
 * so a call is one pass over the observations and one over the cells whatever the network: the levels of the plan play
 * no part, and the result does not depend on them.  With the diagonal observation errors of this library, taking a
 * cell's local observations one at a time and carrying the local observation priors that are still to come along is the
 * Kalman update with R_loc = diag(r_o / rho_o(c)): the analysis mean and variance at the cell are the LETKF's in exact
 * arithmetic, and independent of the order of the observations.  Only + - * / sqrt: fp64 IEEE, no FMA contraction,
 * every product rounded, every sum a running sum from +0 in member order k = 0 .. M-1.
 * assimilate_local: forecast members, truth_member, inflation, record and tol (0: no background check) as in
 *   csim_ensemble_assimilate_screened; the call only enqueues on the ensemble's stream.  Point and linear networks.
 *   1. Screening: the status bytes exactly as in csim_ensemble_assimilate_screened, (hb, vb) from the state before the
 *      inflation.  The used observations are those with status CSIM_OBS_USED (all, when nothing is screened).
 *   2. Inflation: lambda != 1 as in csim_ensemble_assimilate, on every interior cell.
 *   3. Observation priors: for every used observation o and forecast member k, h_{o,k} = the operator value from the
 *      inflated state: the observed cell of a point observation (its bits), sum_s w_s x_k(anchor + tap s) of a linear
 *      one as in csim_obs_network_create_linear.
 *   4. Cell pass: for every interior cell c = (i_c, j_c), L(c) = the used observations o with |i_c - i_o| <= lx,
 *      |j_c - j_o| <= ly, rho_o(c) = rho[j_c - j_o + ly][i_c - i_o + lx] > 0 and r_o / rho_o(c) finite, taken in
 *      increasing input index.  With z_k = x_k(c) and private copies w_{o,k} = h_{o,k}:
 *
 *          for o in L(c), in order:
 *              re = r_o / rho_o(c)
 *              hbar = (sum_k w_{o,k}) / M;   h'_k = w_{o,k} - hbar;   p = (sum_k h'_k h'_k) / (M-1)
 *              d = p + re;   alpha = 1 / (1 + sqrt(re / d));   delta = y_o - hbar
 *              for the target v = z, and then v = w_q for every q in L(c) after o:
 *                  vbar = (sum_k v_k) / M;   v'_k = v_k - vbar;   cov = (sum_k v'_k h'_k) / (M-1)
 *                  g = cov / d;   beta = alpha g;   v_k <- v_k + (g delta - beta h'_k)
 *          x_k(c) <- z_k
 *
 *      A cell with empty L(c) is not written and keeps its bits.  Ghost rings, the other ping-pong buffer and member t
 *      are never touched.  At the cell of a lone point observation rho = 1 and the members are those of
 *      csim_ensemble_assimilate bit for bit.
 *   5. record = 1 appends the two log records of csim_ensemble_assimilate_screened, with
 *      (ha, va) taken after the cell pass, and leaves the network in the same "last analysis was recorded" state:
 *      fetch, log, screen_log, status and impact_capture behave as after a recorded serial analysis.
 *   Limits (resource bounds of the cell pass): with max_local = the largest number of observations whose window
 *   rectangle, clipped to the interior, contains one cell (masks and rho ignored), max_local <= CSIM_LOCAL_MAX_OBS,
 *   max_local M <= CSIM_LOCAL_MAX_DOUBLES (32 KiB of private priors per cell) and nobs M <=
 *   CSIM_LOCAL_MAX_PRIOR_DOUBLES; beyond them CSIM_ERR_UNSUPPORTED (also where the lookup of step 4 would exceed 2^31
 *   entries).  The other errors are those of csim_ensemble_assimilate_screened, in its order and first.  Every error is
 *   raised before anything is enqueued and leaves members, values, mask, logs and diagnostics as they were.
 * local_info: *max_local of the network, computed at the first call and kept.
 * local_count (host-only, needs no device): the rectangle count above for nobs >= 0 observations at interior cells
 *   (i, j) with half-widths lx, ly >= 0 (either may exceed the grid): count (may be NULL) gets ny x nx values,
 *   row-major, cell (i, j) at (j - 1) nx + (i - 1); *max_local (may be NULL) their maximum, 0 without observations.
 *   CSIM_ERR_ARG for nx or ny < 1, nobs < 0, lx or ly < 0, a null array with nobs > 0, a cell outside the interior. */
#define CSIM_LOCAL_MAX_OBS 64
#define CSIM_LOCAL_MAX_DOUBLES 4096
#define CSIM_LOCAL_MAX_PRIOR_DOUBLES (1L << 26)
int csim_ensemble_assimilate_local(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                   int record, double tol);
int csim_obs_network_local_info(csim_obs_network* n, int* max_local);
int csim_obs_local_count(int nx, int ny, int nobs, const int* i, const int* j, int lx, int ly, int* count,
                         int* max_local);
/* ensemble space: the M x M space spanned by the forecast members' perturbations.  Two primitives, both one pass over
 * the members, and two composites on the host.  M forecast members in forecast order, truth member t stepped over
 * (truth_member = -1: none), 1 <= M <= CSIM_ESPACE_MAX_MEMBERS (more: CSIM_ERR_UNSUPPORTED).  Every * + - / below is
 * one IEEE fp64 operation, no FMA contraction; running sums start from +0 and take their terms in the stated order.
 * Perturbations of a cell:  centered = 1:  s = +0; s = s + x_k (k = 0 .. M-1); m = s / M; p_k = x_k - m.
 *                           centered = 0:  p_k = x_k.
 * gram: G[a][b] = sum over the interior cells of p_a p_b, M x M row-major; synchronous, writes no member.  The order:
 *   interior cells are numbered e = (j-1) nx + (i-1); segment q holds cells 64 q .. 64 q + 63 (the last may be short),
 *   nseg = ceil(nx ny / 64); Gc = min(nseg, cap), cap = 1024 for M <= 64, 256 for M <= 128, 64 above.  Class g owns
 *   segments g, g + Gc, g + 2 Gc, ...; for each (a, b) the class partial is one running sum over the class's cells in
 *   increasing e, carried across its segments: acc = acc + (p_a * p_b).  G[a][b] = partial_0 + partial_1 + ... +
 *   partial_{Gc-1}, starting from partial 0.  Nothing in this order depends on the launch geometry; G is symmetric
 *   bit for bit.  gram_plan (host-only, needs no device): *nseg and *classes = Gc (either may be NULL).
 * project: out_r = s_r on every cell of the reference layout (ny+2) x (nx+2), ghost ring included, K dense fields,
 *   1 <= K <= M, W is M x K row-major:  s_r = +0; s_r = s_r + p_k * W[k K + r]  (k = 0 .. M-1).  Synchronous.
 * transform: replaces the forecast members by a linear combination of them, on every interior cell (ghost ring and
 *   member t keep their bits); W is M x M row-major, s_r as above with K = M:
 *     centered = 1:  d = +0; d = d + p_k * wbar[k] (k in order); m' = m + d (wbar NULL: m' = m);  x'_r = m' + s_r
 *     centered = 0:  x'_r = s_r;  a non-NULL wbar is CSIM_ERR_ARG
 *   All M values of a cell are read before any is written.  With centered = 0 and W a 0/1 selection matrix the result
 *   is an exact copy or resampling of members (up to the sign of a zero).  The call only enqueues on the ensemble's
 *   stream: W and wbar are copied to staging before it returns, so run -> gram -> transform -> run needs no
 *   synchronisation beyond the one gram makes.
 * dot: the adjoint of project, the inner product of every member's perturbation with K fields, 1 <= K <=
 *   CSIM_DOT_MAX_FIELDS.  fields: K host fields in the reference layout (ny+2) x (nx+2), one after the other; only the
 *   interior is read (ghost values may be NaN), and it is copied before any kernel runs.  out is M x K row-major:
 *   out[k K + r] = sum over the interior cells of p_k f_r.  Synchronous, writes no member.  The order is gram's, word
 *   for word: the same cells e, segments, Gc = min(nseg, cap) with the cap taken from M alone, class g owning segments
 *   g, g + Gc, ...; for each (k, r) the class partial is one running sum over the class's cells in increasing e, carried
 *   across its segments: acc = acc + (p_k * f_r); out[k K + r] = partial_0 + partial_1 + ... + partial_{Gc-1}.
 *   csim_ensemble_gram_plan is its plan; nothing depends on the launch geometry.  So with centered = 0 and f_r the
 *   field of forecast member b, out[k K + r] is gram(centered = 0)[k][b] bit for bit.
 *   Errors, in this order, before anything is enqueued: CSIM_ERR_ARG for a null ensemble; those of this block for
 *   truth_member, M and centered; CSIM_ERR_ARG for K outside 1 .. CSIM_DOT_MAX_FIELDS, a null fields or out, and a
 *   non-finite interior value of a field.
 * sym_eigen (host-only): the eigenvalues and vectors of the symmetric n x n matrix A (row-major; the upper triangle is
 *   read), 1 <= n <= CSIM_SYM_EIGEN_MAX_N, by the cyclic Jacobi method.  a = A (kept symmetric entry by entry),
 *   v = I.  A sweep takes the pairs p < q in row-cyclic order (p = 0 .. n-2, q = p+1 .. n-1); with g = |a_pq|:
 *     a_pq == 0: nothing;  |a_pp| + g == |a_pp| and |a_qq| + g == |a_qq|: a_pq <- 0, no rotation;  otherwise
 *     h = a_qq - a_pp;  |h| + g == |h|: t = a_pq / h;  else theta = (0.5 h) / a_pq,
 *     t = 1 / (|theta| + sqrt(theta theta + 1)), negated for theta < 0;
 *     c = 1 / sqrt(t t + 1);  s = t c;  tau = s / (1 + c);  h = t a_pq;  a_pp <- a_pp - h;  a_qq <- a_qq + h;  a_pq <- 0;
 *     for j != p, q (j ascending), x = a_jp, y = a_jq:  a_jp <- x - s (y + x tau);  a_jq <- y + s (x - y tau);
 *     for every j, the same with x = v_jp, y = v_jq.
 *   It stops before a sweep that finds every off-diagonal element exactly zero, or after CSIM_SYM_EIGEN_MAX_SWEEPS
 *   sweeps; *sweeps (may be NULL) = sweeps made.  lambda: the diagonal, sorted descending, ties to the lower original
 *   index; V (n x n row-major): column r is the vector of lambda[r], negated if its first component of largest
 *   magnitude is negative.  CSIM_ERR_ARG: n < 1, a non-finite entry; CSIM_ERR_UNSUPPORTED: n above the limit.
 * sym_eigen_ordered (host-only): the same with the pairs of a sweep in the order `order`.  CSIM_EIGEN_ROWS is the order
 *   above and gives csim_sym_eigen's bits.  CSIM_EIGEN_ROUND_ROBIN is a parallel order: a sweep is a sequence of steps,
 *   each a set of disjoint pairs, and it is the order of the device solver below.
 *   Pairing: m = n rounded up to even; a sweep is the steps t = 0 .. m-2; step t has the slots k = 0 .. m/2-1:
 *     slot 0 = {m-1, t};  slot k >= 1 = {(t+k) mod (m-1), (t-k) mod (m-1)};  within a slot p < q.
 *     Every pair p < q < m is in exactly one slot of a sweep.  A slot with q >= n (odd n: slot 0, whose p = t) is idle:
 *     it has no rotation and its lone index p is rotated by nobody.
 *   Parameters: per active slot, from a_pp, a_qq and a_pq as the matrix stands at the start of the step, by the decisions
 *     and formulas above: a_pq == 0: no rotation;  the "tiny" test: a_pq <- a_qp <- 0 and no rotation;  otherwise t, c,
 *     s, tau and h = t a_pq as above, a_pp <- a_pp - h, a_qq <- a_qq + h, a_pq <- a_qp <- 0.  These three entries belong
 *     to the slot alone.
 *   Applying the step: with rot(x, y; s, tau): xn = x - s (y + x tau), yn = y + s (x - y tau), for every two slots K < L
 *     (by slot number) the block a[{p_K, q_K}][{p_L, q_L}] is first rotated as rows by K, that is rot(a[p_K][j],
 *     a[q_K][j]) with K's (s, tau) for j = p_L and j = q_L, then the results are rotated as columns by L, that is
 *     rot(a[i][p_L], a[i][q_L]) with L's (s, tau) for i = p_K and i = q_K; the four results are stored and mirrored
 *     into a[j][i].  A slot without a rotation applies none, so a block of two such slots keeps its bits; against the
 *     lone index of an idle slot only the other slot's rotation acts, on the two entries that exist.  For every slot with
 *     a rotation, rot(v_jp, v_jq) for every j as above.  All of these act on disjoint entries, so the result depends on
 *     no order among them: taking the slots of a step one after the other, each as one pair of the row order's loop
 *     body, gives the same bits, and that is how the host computes it.  a is symmetric entry by entry after every step.
 *   Stop, sort and sign as above.  CSIM_ERR_ARG also for an unknown order.
 * sym_eigen_batch_gpu: `batch` matrices A[b] (n x n row-major, one after the other) by the round-robin order on the
 *   device, one workgroup per matrix, 1 <= n <= CSIM_SYM_EIGEN_MAX_N, 1 <= batch <= CSIM_SYM_EIGEN_MAX_BATCH.  Host arrays
 *   in and out, synchronous; the call creates and frees the stream and the device memory it needs (at most 512 MiB at a
 *   time) and needs no ensemble.  lambda[b], V[b], sweeps[b] (may be NULL) are bit for bit those of
 *   csim_sym_eigen_ordered(CSIM_EIGEN_ROUND_ROBIN) on A[b];  status[b] (may be NULL) is CSIM_EIGEN_OK, or
 *   CSIM_EIGEN_NONFINITE: A[b] has a non-finite entry, lambda[b] and V[b] are NaN and sweeps[b] = 0 (the other matrices
 *   are not affected), or CSIM_EIGEN_NOT_CONVERGED: all CSIM_SYM_EIGEN_MAX_SWEEPS sweeps were made (sweeps[b] says the
 *   same on the host); lambda and V are then the current diagonal and vectors, as on the host.
 *   form: 0, or the storage form of the working matrices to force: 1 = a and v in LDS (n <= 96), 2 = a in LDS and v in
 *   global memory (n <= 128), 3 = both in global memory (any n); 0 takes the first that admits n.  Every form gives the
 *   same bits.  sym_eigen_device_form (host-only): *chosen = the form taken for (n, form), *max_n = the largest n that
 *   `form` admits (either may be NULL); CSIM_ERR_UNSUPPORTED when the form does not admit n.
 *   Not built: a solver that spans workgroups, and eofs on the device order.
 * eofs: the leading patterns of the ensemble's spread, 1 <= n_modes <= M - 1:  G = gram(centered = 1);
 *   (lam, V) = sym_eigen(G);  lambda[r] = lam_r;  mode r is null when lam_r <= (M 2^-52) lam_0 or lam_r <= 0, else
 *   W[k][r] = V[k][r] / sqrt(lam_r) and pcs[k n_modes + r] = V[k][r] * sqrt(lam_r);  patterns (NULL: not wanted) =
 *   project(centered = 1, K = n_modes, W): n_modes dense fields, so that p_k = sum_r pcs[k][r] pattern_r on every cell
 *   up to rounding.  A null mode has zero pcs and a zero pattern; *n_valid (may be NULL) counts the others.
 * space_check (host-only): the argument checks of the four calls for an ensemble of `members` members, in the order
 *   truth_member, M, centered, K (0: not a projection), wbar, n_modes (0: not eofs). */
#define CSIM_ESPACE_MAX_MEMBERS 256
#define CSIM_DOT_MAX_FIELDS 16
#define CSIM_SYM_EIGEN_MAX_N 256
#define CSIM_SYM_EIGEN_MAX_SWEEPS 64
#define CSIM_SYM_EIGEN_MAX_BATCH 65535
#define CSIM_EIGEN_ROWS 0
#define CSIM_EIGEN_ROUND_ROBIN 1
#define CSIM_EIGEN_OK 0
#define CSIM_EIGEN_NONFINITE 1
#define CSIM_EIGEN_NOT_CONVERGED 2
int csim_ensemble_gram(csim_ensemble* e, int truth_member, int centered, double* G);
int csim_ensemble_gram_plan(int M, int nx, int ny, long* nseg, int* classes);
int csim_ensemble_project(csim_ensemble* e, int truth_member, int centered, int K, const double* W, double* out);
int csim_ensemble_transform(csim_ensemble* e, int truth_member, int centered, const double* W, const double* wbar);
int csim_ensemble_dot(csim_ensemble* e, int truth_member, int centered, int K, const double* fields, double* out);
int csim_sym_eigen(int n, const double* A, double* lambda, double* V, int* sweeps);
int csim_sym_eigen_ordered(int n, const double* A, int order, double* lambda, double* V, int* sweeps);
int csim_sym_eigen_batch_gpu(int n, int batch, const double* A, double* lambda, double* V, int* sweeps, int* status,
                             int form);
int csim_sym_eigen_device_form(int n, int form, int* chosen, int* max_n);
int csim_ensemble_eofs(csim_ensemble* e, int truth_member, int n_modes, double* lambda, double* pcs, double* patterns,
                       int* n_valid);
int csim_ensemble_space_check(int members, int truth_member, int centered, int K, int has_wbar, int n_modes);
/* ETKF: the global ensemble transform Kalman filter on a network, from an observation-space Gram matrix.  M forecast
 * members in forecast order, truth member t stepped over, 2 <= M <= CSIM_ESPACE_MAX_MEMBERS (more:
 * CSIM_ERR_UNSUPPORTED).  Every * + - / sqrt below is one IEEE fp64 operation, no FMA contraction; running sums start
 * from +0 and take their terms in the stated order.
 * obs_gram: reduces Y = H X' of a whole network (point or linear) to the ensemble space; synchronous.  The network must
 *   have values (else CSIM_ERR_STATE); an observation is used when the network's current mask leaves it active; no
 *   background check is made and nothing of the network is written: no status byte, no flag, no log.  Per plan position
 *   q, the network's own order (level, then input index; csim_ensemble_assim_plan):
 *       h_k = the operator value of forecast member k: the point cell's bits, or the tap sum of a linear observation
 *             as in csim_obs_network_create_linear
 *       s = sum_k h_k;   hb = s / M;   z_k = (h_k - hb) / sr_q  (k < M);   z_M = (y_q - hb) / sr_q
 *       e_k = (y_q - h_k) / sr_q
 *   with sr_q = sqrt(r_q) as the network stores it.  An observation that is not used is not read: all its z and e are
 *   +0.  A (NULL: not wanted) is (M+1) x (M+1) row-major, A[a][b] = sum_q z_a z_b, symmetric bit for bit: C = A[:M,:M]
 *   = Y^T R^-1 Y, c = A[:M,M] = Y^T R^-1 (y - hb), A[M][M] the innovation chi^2.  loglik (NULL: not wanted and not
 *   computed) gets M values, loglik[k] = sum_q e_k e_k: a particle weight is exp(-loglik[k] / 2), normalised by the
 *   caller.  *n_used (may be NULL): the used observations.  The order of every sum is that of csim_ensemble_gram with plan
 *   positions in place of cells: segment s holds plan positions 64 s .. 64 s + 63, nseg = ceil(nobs / 64), Gc =
 *   min(nseg, cap) with gram's cap; class g owns segments g, g + Gc, ... and keeps one running sum per entry in
 *   increasing q, carried across its segments: acc = acc + (z_a * z_b), and acc = acc + (e_k * e_k); the result is
 *   partial_0 + partial_1 + ... + partial_{Gc-1}, starting from partial 0.  Nothing depends on the launch geometry.
 *   obs_gram_plan (host-only): *nseg and *classes = Gc (either may be NULL) for M >= 2 and nobs >= 1.
 * etkf_weights (host-only): the symmetric square-root ETKF of Hunt et al. 2007 with the multiplicative inflation taken
 *   in ensemble space.  A as above, C = A[:M,:M]; W is M x M and symmetric bit for bit, wbar and gamma M values; every
 *   output may be NULL.
 *       rho = inflation * inflation;   kappa = (double)(M-1) / rho;   (lam, V) = csim_sym_eigen(M, C)
 *       G_r = lam_r > 0 ? lam_r : +0;   f_r = 1 / (kappa + G_r);   g_r = sqrt((double)(M-1) * f_r)
 *       u_r = sum_a V[a][r] * A[a][M]  (a ascending);   wbar[a] = sum_r V[a][r] * (f_r * u_r)  (r ascending)
 *       W[a][b] = sum_r (V[a][r] * g_r) * V[b][r]  for a <= b (r ascending), mirrored into W[b][a]
 *       gamma[r] = G_r;   *dfs = sum_r G_r * f_r, the degrees of freedom for signal;   *sweeps: those of sym_eigen
 *   CSIM_ERR_ARG: M < 2, inflation < 1 or not finite, A NULL or with a non-finite entry; CSIM_ERR_UNSUPPORTED: M above
 *   the limit.  transform(centered = 1, W, wbar) is then the analysis: mean xb + X' wbar, perturbations X' W.
 *   etkf_weights_ordered: the same on csim_sym_eigen_ordered(M, C, order); order CSIM_EIGEN_ROWS gives
 *   csim_etkf_weights' bits; CSIM_ERR_ARG also for an unknown order.
 * assimilate_etkf: the analysis from these pieces; arguments and errors as csim_ensemble_assimilate_screened, in its
 *   order and first, then M <= CSIM_ESPACE_MAX_MEMBERS (more: CSIM_ERR_UNSUPPORTED).
 *   1. Screening exactly as in csim_ensemble_assimilate_screened: (hb, vb), the mask and the background check write the
 *      status bytes, so status, screen_log and fetch behave as after csim_ensemble_assimilate_network.
 *   2. A = obs_gram over the observations whose status is CSIM_OBS_USED (all, when nothing is screened); the call
 *      waits for it.  A non-finite entry of A: CSIM_ERR_STATE, the members untouched and no record appended.
 *   3. (W, wbar) = etkf_weights(A, inflation);  transform(centered = 1, W, wbar) is enqueued.  With no used
 *      observation and inflation == 1 no transform is launched and the members keep their bits.
 *   4. record = 1 appends the two log records as csim_ensemble_assimilate_screened does, (ha, va) taken after the
 *      transform.
 *   Where tol = 0 the members are bit for bit those of obs_gram -> etkf_weights -> transform through the public calls.
 *   The filter is global: the network's loc plays no part.  No field is inflated: the inflation acts only through
 *   kappa, which equals the other analyses' inflation of the prior perturbations up to rounding, not bit for bit.
 *   etkf_info: n_used, chi2 = A[M][M], dfs and gamma (M values; *n_gamma = M) of the ensemble's last completed
 *   assimilate_etkf, every pointer may be NULL; CSIM_ERR_STATE when there is none, or when the last call that passed
 *   its argument and state checks failed after them.
 * assimilate_etkf_device: the same analysis without a copy or a wait, for cycling on the device: checks, screening and
 *   record as assimilate_etkf; then the obs_gram kernels, the device eigensolver on C (one workgroup; the ensemble's
 *   option "eigen_form"), a kernel that computes etkf_weights_ordered(order = CSIM_EIGEN_ROUND_ROBIN) operation by
 *   operation from A, lam and V on the device, and the transform are enqueued on the ensemble's stream.  Without record
 *   the call only enqueues.  The members are bit for bit those of obs_gram -> etkf_weights_ordered(round robin) ->
 *   transform through the public calls; they differ from assimilate_etkf's in the last bits, as the two orders do.
 *   With no used observation and inflation == 1, or with a non-finite entry of A, the transform kernel reads that from
 *   the device record and returns at once: the members keep their bits.  A non-finite A cannot fail this call: the
 *   following etkf_info returns CSIM_ERR_STATE, and with record = 1 the cycle's log records have been appended, (ha, va)
 *   taken from the unchanged members.  2 <= M <= CSIM_ESPACE_MAX_MEMBERS; CSIM_ERR_UNSUPPORTED also when the eigen_form
 *   that is set does not admit M.
 *   etkf_info after it waits for the stream and fetches the record.  etkf_info2 is etkf_info with two more outputs
 *   (either may be NULL): *sweeps, the solver's sweeps, and *status, CSIM_EIGEN_OK or CSIM_EIGEN_NOT_CONVERGED (the
 *   analysis was made with the current diagonal, as the host makes it); after assimilate_etkf both are 0.
 * The forecast impact after an ETKF: impact_capture after a recorded one, then csim_ensemble_obs_impact_global, the
 *   estimate whose premise this filter satisfies exactly (see there), on the host path and the device path alike.
 * Not built: _begin / _wait forms, more than CSIM_ESPACE_MAX_MEMBERS members, and a resampling particle filter on top
 * of loglik. */
int csim_ensemble_obs_gram(csim_ensemble* e, csim_obs_network* n, int truth_member, double* A, double* loglik,
                           long long* n_used);
int csim_obs_gram_plan(int M, int nobs, long* nseg, int* classes);
int csim_etkf_weights(int M, const double* A, double inflation, double* W, double* wbar, double* gamma, double* dfs,
                      int* sweeps);
int csim_ensemble_assimilate_etkf(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                  int record, double tol);
int csim_ensemble_etkf_info(const csim_ensemble* e, long long* n_used, double* chi2, double* dfs, double* gamma,
                            int* n_gamma);
int csim_etkf_weights_ordered(int M, const double* A, double inflation, int order, double* W, double* wbar,
                              double* gamma, double* dfs, int* sweeps);
int csim_ensemble_assimilate_etkf_device(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                         int record, double tol);
int csim_ensemble_etkf_info2(csim_ensemble* e, long long* n_used, double* chi2, double* dfs, double* gamma,
                             int* n_gamma, int* sweeps, int* status);
/* 4D-ETKF: observations assimilated at their own times in the window (Hunt et al. 2004, 2007).  A network has time
 * slots 0 .. CSIM_OBS_MAX_SLOTS - 1 and every observation belongs to one.  While the forecast runs the caller holds a
 * slot when the model reaches its time: h_k of every forecast member for the slot's observations goes into rows of the
 * network's own, which stay across run calls.  At the end of the window a held analysis forms the ETKF's weights from the
 * rows instead of the current state and applies them to the members and to the rows.  Every * + - / sqrt is one IEEE
 * fp64 operation, no FMA contraction; running sums start from +0 in the stated order.
 * slots_present (host-only): *mask gets bit s for every slot s that occurs among the nobs values (slot NULL: bit 0);
 *   CSIM_ERR_ARG for a value outside 0 .. CSIM_OBS_MAX_SLOTS - 1, nobs < 1 or a NULL mask.  The rule of the library's own
 *   bookkeeping: a network is "held" ("observed") when every bit of this mask is.
 * set_slots: nobs values in input order, NULL: all 0, which is also a new network's state.  CSIM_ERR_ARG for a value out
 *   of range, before anything changes.  Forgets which slots are held and which are observed; enqueues an upload only.
 * hold: slot = -1 means every observation.  For every plan position q of the slot, whatever the mask and the status bytes
 *   say, H[q][k] = h_k of obs_gram above (the point cell's bits, or the tap sum in tap order from +0) of the M forecast
 *   members in forecast order, from the current buffer after everything enqueued so far.  Rows of other slots keep their
 *   bits; a slot without observations is a no-op that still counts as held.  Enqueues only.  The rows are nobs x M
 *   doubles, [plan position][member], the layout of the local analysis's priors, reserved at the first hold.
 *   CSIM_ERR_ARG: slot or truth_member out of range; CSIM_ERR_UNSUPPORTED: nobs M above CSIM_LOCAL_MAX_PRIOR_DOUBLES, or M
 *   outside 2 .. CSIM_ESPACE_MAX_MEMBERS.  A hold with another (M, truth_member) than the rows already held forgets those
 *   rows first.
 * observe_slot: csim_obs_network_observe restricted to the observations of the slot: xt_o and y_o get the bits that
 *   observe would give them at this moment (the noise depends on the input index o alone), every other observation
 *   keeps y and xt.  The network has values once set_values or observe was called, or once every slot that occurs has
 *   been observed since set_slots (and since the last set_values); that it has a truth follows the same rule.
 * held: waits for the stream; the rows in input order, nobs x M (H NULL: not wanted), *M and *truth_member (-1: none) of
 *   the hold (either may be NULL).  CSIM_ERR_STATE when not every slot that occurs is held; after a held analysis it
 *   returns the transformed rows until the next hold.
 * obs_gram_held: obs_gram above word for word with h_k = H[q][k]: the mask, an observation that is not used not being
 *   read, the segment, class and fold order and the symmetry; M and t are those of the hold.  CSIM_ERR_STATE when not
 *   every slot that occurs is held, or when the network has no values.  Writes nothing of the network.  The result does
 *   not depend on the option obs_gram_form.
 * assimilate_etkf_held: the steps of assimilate_etkf (device = 0) or assimilate_etkf_device (device = 1) with these
 *   differences: (hb, vb) of the screening and the record are mv of csim_ensemble_relax over the M values of the held
 *   row, not of the state; A is obs_gram_held over the used observations; the same (W, wbar) is applied twice, to the
 *   members by transform(centered = 1), and to every held row, which is treated exactly as one cell's M members are
 *   under transform(centered = 1), all M values read before any is written; where the analysis launches no transform (no
 *   used observation and inflation 1; on the device path the status record says nothing to do or non-finite) the rows
 *   keep their bits too; with record = 1, (ha, va) are mv of the transformed rows.  So after the call the rows are the
 *   analysis in observation space at report time.  Errors: the analysis's own, first and in their order; then
 *   CSIM_ERR_STATE when not every slot that occurs is held, or when truth_member or M differ from the hold's.  A held
 *   analysis ends the window: afterwards no slot counts as held, and a second one without new holds is CSIM_ERR_STATE.
 *   On the host path a call that fails, the non-finite A among its errors, has not ended the window: the rows and the
 *   holds stand, and the call may be repeated without a new hold, after set_active for instance; on the device path the
 *   window is over once the call has returned CSIM_OK, also where etkf_info later reports a non-finite A.
 *   etkf_info and etkf_info2 work as after the calls above.  csim_obs_network_impact_capture after a held analysis is
 *   CSIM_ERR_STATE: a_k at report time is not what the impact's estimate takes.
 * Not built: the held form of the serial, local and LETKF analyses, and forecast impact for held observations. */
#define CSIM_OBS_MAX_SLOTS 64
int csim_obs_slots_present(int nobs, const int* slot, unsigned long long* mask);
int csim_obs_network_set_slots(csim_obs_network* n, const int* slot);
int csim_obs_network_hold(csim_obs_network* n, int slot, int truth_member);
int csim_obs_network_observe_slot(csim_obs_network* n, int slot, int source_member, unsigned long long seed,
                                  unsigned draw, int noise);
int csim_obs_network_held(csim_obs_network* n, double* H, int* M, int* truth_member);
int csim_ensemble_obs_gram_held(csim_ensemble* e, csim_obs_network* n, double* A, double* loglik, long long* n_used);
int csim_ensemble_assimilate_etkf_held(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member,
                                       int record, double tol, int device);
/* LETKF: the ETKF made local (Hunt et al. 2007): ensemble-space weights from the observations near a point, with the
 * network's localisation in the observation error, computed on a coarse lattice of analysis nodes and interpolated to
 * the cells (Yang et al. 2009).  The node spacing s trades cost against locality; s = 1 has a node on every cell and is
 * the full LETKF.  Every * + - / sqrt below is one IEEE fp64 operation, no FMA contraction; running sums start from +0
 * and take their terms in the stated order.  The call only enqueues on the ensemble's stream.
 * assimilate_letkf: arguments and errors as csim_ensemble_assimilate_local, in its order and first; then spacing >= 1
 *   (else CSIM_ERR_ARG); then the limits, beyond which CSIM_ERR_UNSUPPORTED: 2 <= M <= CSIM_ESPACE_MAX_MEMBERS, nobs M <=
 *   CSIM_LOCAL_MAX_PRIOR_DOUBLES, nodes <= CSIM_LETKF_MAX_NODES, the bytes of csim_letkf_plan <= CSIM_LETKF_MAX_BYTES,
 *   and the option "eigen_form" that is set admits M.  Every error is raised before anything is enqueued.
 *   CSIM_LOCAL_MAX_OBS and CSIM_LOCAL_MAX_DOUBLES do not apply: any number of windows may cover a cell.
 *   1. Screening, inflation of the field and the observation priors h_{o,k}: steps 1 to 3 of
 *      csim_ensemble_assimilate_local.  The inflation acts on the field; the weights below take inflation 1.
 *   2. Nodes: along x, nax = 1 for nx = 1, else ceil((nx - 1) / s) + 1, node a at the interior cell
 *      i_a = min(1 + a s, nx); the same along y; node (a, b) has index b nax + a.
 *   3. Node Gram matrix: L(g) of the node's cell is exactly L(c) of csim_ensemble_assimilate_local (used, inside the
 *      window, rho_o > 0, r_o / rho_o finite; increasing input index).  Per o in L(g):
 *          re = r_o / rho_o;  sre = sqrt(re);  s = sum_k h_{o,k} (k ascending);  hb = s / M
 *          z_k = (h_{o,k} - hb) / sre  (k < M);   z_M = (y_o - hb) / sre
 *      A_g[a][b], (M+1) x (M+1), is one running sum over L(g) in order: acc = acc + (z_a * z_b); symmetric bit for bit.
 *      count_g = |L(g)|.
 *   4. Node weights: count_g = 0: status CSIM_LETKF_IDLE; else a non-finite entry of A_g: CSIM_LETKF_NONFINITE; for
 *      both W_g and wbar_g are not defined and never read, and dfs_g = +0, sweeps_g = 0.  Otherwise
 *      (W_g, wbar_g, dfs_g, sweeps_g) = csim_etkf_weights_ordered(M, A_g, 1.0, CSIM_EIGEN_ROUND_ROBIN) bit for bit, computed
 *      by the batched device eigensolver (option "eigen_form") and a batched form of the weights kernel; status
 *      CSIM_LETKF_OK, or CSIM_LETKF_NOT_CONVERGED when the solver made all its sweeps (the weights are then taken from
 *      the current diagonal and vectors, as on the host).
 *   5. Cell pass, every interior cell (i, j):  with nax >= 2, a = min((i - 1) / s, nax - 2) and
 *      tx = (double)(i - i_a) / (double)(i_{a+1} - i_a); with nax = 1, a = 0 and tx = +0; likewise b and ty from j.
 *      ax = 1 - tx; ay = 1 - ty.  The nodes n = 0 .. 3 are (a, b), (a+1, b), (a, b+1), (a+1, b+1) with the weights
 *      beta_n = ay ax, ay tx, ty ax, ty tx.  A node with beta_n == 0 is skipped and not read (with one node along an
 *      axis the upper node does not exist and always has beta = 0).  If every remaining node is IDLE or NONFINITE the
 *      cell is not written and keeps its bits.  Otherwise, with m and p_k of transform(centered = 1):
 *          a remaining node that is IDLE or NONFINITE:  d_n = +0;  s_{r,n} = p_r
 *          any other:  d_n = sum_k p_k * wbar_n[k];  s_{r,n} = sum_k p_k * W_n[k M + r]   (k ascending)
 *          c_r = +0;  c_r = c_r + beta_n * (d_n + s_{r,n})  over the remaining nodes in order;   x'_r = m + c_r
 *      All M values of a cell are read before any is written.  Ghost ring, member t and the other ping-pong buffer are
 *      never touched.
 *   6. record = 1: as step 5 of csim_ensemble_assimilate_local; fetch, log, screen_log, status and impact_capture
 *      behave as after a recorded local analysis.  The forecast impact after an LETKF is the localised
 *      csim_ensemble_obs_impact, not the global one.  In the OSSE of DESIGN 7z (21 members of 33 x 17, 40 stations,
 *      six steps, eight seeds, on the CPU restatements) its total has the sign of the actual change of the forecast
 *      error for every seed; total / actual is 0.86 .. 0.90 at spacing 1 and 2.19 .. 3.25 at spacing 4, where the
 *      interpolated weights are not the gain the estimate assumes: with a coarse lattice take the sign and the ranking
 *      of the observations from it, not the size.
 *      csim_ensemble_etkf_info is not affected by this call.
 *   With s = 1 every cell is a node with beta = (1, 0, 0, 0) and the analysis mean and variance are those of
 *   csim_ensemble_assimilate_local in exact arithmetic.
 * letkf_info: the ensemble's last assimilate_letkf, per node, row-major nay x nax: dfs (the degrees of freedom for
 *   signal), count (the local observations used), sweeps (the solver's) and status (CSIM_LETKF_*); *nax, *nay the
 *   lattice.  Every pointer may be NULL; the arrays have csim_letkf_nodes' nax nay entries.  Waits for the stream.
 *   CSIM_ERR_STATE when there was no LETKF, or when a node's status is CSIM_LETKF_NONFINITE (the arrays are filled all
 *   the same).
 * letkf_nodes, letkf_blend, letkf_plan (host-only, need no device): nx, ny >= 1 and spacing >= 1, else CSIM_ERR_ARG.
 *   nodes: *nax, *nay, and the nodes' cells xi[0 .. nax-1], yj[0 .. nay-1] (every pointer may be NULL).
 *   blend: for the interior cell (i, j) the four node indices and beta of step 5; a node that does not exist (one node
 *   along an axis) is reported as its lower neighbour, with beta = +0.
 *   plan: for M >= 2 forecast members *nodes = nax nay and *bytes, the device storage of the nodes of one call with
 *   "eigen_form" 0 (a forced form may keep the solver's working matrices in global memory on top); M above
 *   CSIM_ESPACE_MAX_MEMBERS: CSIM_ERR_UNSUPPORTED.
 * Cost (one MI355X, 63 forecast members, loc = 8 cells): the batched eigensolver dominates (80 % at spacing
 *   8), and the analysis is slower than the serial filter on every network measured: 7.4 ms at spacing 8 and 3.8 ms at
 *   16 against 0.94 ms for 1024 random observations on 256^2, 20.0 ms and 8.3 ms against 0.31 ms on 512^2.  64 members
 *   need spacing >= 8 on 512^2 and >= 4 on 256^2, 256 members spacing >= 16 on 256^2 (CSIM_LETKF_MAX_BYTES).  The
 *   analysis mean differs from that of spacing 1 by 6.5 %, 23 % and 62 % of the RMS increment at spacing 4, 8 and 16.
 * Not built: more than CSIM_LETKF_MAX_NODES nodes in one call (the lattice taken in parts). */
#define CSIM_LETKF_MAX_NODES 65535
#define CSIM_LETKF_MAX_BYTES (1LL << 30)
#define CSIM_LETKF_OK 0
#define CSIM_LETKF_IDLE 1
#define CSIM_LETKF_NONFINITE 2
#define CSIM_LETKF_NOT_CONVERGED 3
int csim_ensemble_assimilate_letkf(csim_ensemble* e, csim_obs_network* n, double inflation, int truth_member, int record,
                                   double tol, int spacing);
int csim_ensemble_letkf_info(csim_ensemble* e, int* nax, int* nay, double* dfs, int* count, int* sweeps, int* status);
int csim_letkf_nodes(int nx, int ny, int spacing, int* nax, int* nay, int* xi, int* yj);
int csim_letkf_blend(int nx, int ny, int spacing, int i, int j, int node[4], double beta[4]);
int csim_letkf_plan(int M, int nx, int ny, int spacing, long* nodes, long long* bytes);
/* options (unknown keys: CSIM_ERR_ARG; "contract": CSIM_ERR_UNSUPPORTED), results never depend on them:
 *   "fuse"        -1 (default) passes of the ensemble depth where the grid allows; 0 / 1 single steps only
 *   "fused_2c"    0/1 (default 1), as for csim_stepper_set_option
 *   "depth_used"  read-only: time steps per pass of the last run (1 = single steps only)
 *   "spatial_grid_max"      0 (default: the kernels' own caps) or 1 .. 65535: workgroups along x of both kernels of
 *                           csim_ensemble_verify_spatial, each of which loops over its cells or tiles
 *   "spatial_member_split"  0 (default: chosen from cells and M) or 1 .. 4096: parts the forecast members of a cell
 *                           are split into in that call's count pass (1: no split; more than M: M)
 *   "perturb_tile_rows"     0 (default: chosen from the grid and M), 8 or 32: interior rows per workgroup tile of
 *                           csim_ensemble_perturb; any other value is CSIM_ERR_ARG
 *   "perturb_member_shares" 0 (default: chosen from the tiles and M) or 1 .. 65535: workgroups that share the forecast
 *                           members of one tile in that call (more than M: M)
 *   "local_tile"            0 (default: chosen from the grid), 4, 8 or 16: cells per side of a tile of the lookup of
 *                           csim_ensemble_assimilate_local; any other value is CSIM_ERR_ARG
 *   "local_pack"            0 (default: as many as fit) or 1 .. 64: cells that one wave of that call's cell pass takes
 *                           together (more than fit beside max_local observations each: as many as fit)
 *   "gram_form"             0 (default: chosen from M) or 1, 2, 3: 1, 2 or 4 blocks of 4 x 4 pairs per lane in the
 *                           class-partial kernel of csim_ensemble_gram; any other value is CSIM_ERR_ARG
 *   "project_form"          0 (default: a cell's members in registers up to M = 64, in LDS above) or 1 (in LDS whatever
 *                           M) in csim_ensemble_project and csim_ensemble_transform; any other value is CSIM_ERR_ARG
 *   "obs_gram_form"         0 (default: chosen from M) or 1, 2, 3: blocks per lane as "gram_form", in the class-partial
 *                           kernel of csim_ensemble_obs_gram and csim_ensemble_assimilate_etkf; any other value is
 *                           CSIM_ERR_ARG
 *   "eigen_form"            0 (default: chosen from M) or 1, 2, 3: the storage form of the device eigensolver in
 *                           csim_ensemble_assimilate_etkf_device (see sym_eigen_batch_gpu); any other value is
 *                           CSIM_ERR_ARG
 *   "letkf_form"            0 (default: a cell's members in registers up to M = 64, in LDS above) or 1 (in LDS whatever
 *                           M) in the cell pass of csim_ensemble_assimilate_letkf; any other value is CSIM_ERR_ARG */
int csim_ensemble_set_option(csim_ensemble* e, const char* key, long value);
int csim_ensemble_get_option(const csim_ensemble* e, const char* key, long* value);
/* host-only pass planner of csim_ensemble_run: out[0] = steps per fused pass (1: none; members with nx or ny below
 * the depth step singly), out[1] = fused passes, out[2] = single steps after them (nsteps = out[1] out[0] + out[2]) */
int csim_ensemble_plan(int nsteps, int nx, int ny, int fuse, int out[3]);
/* host-only: the launch (upwind-sign class 0..8) a member with these parameters belongs to, and the number of
 * launches per pass of a batch with the given classes */
int csim_ensemble_sign_class(double dx, double dy, double D, double dt, double vx, double vy, int fused_2c, int* cls);
int csim_ensemble_classes(int members, const int* cls, int* nlaunches);

#ifdef __cplusplus
}
#endif
#endif /* CSIM_H */
