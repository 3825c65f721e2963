// sweep_core.hpp — the device code that the single stepper (sweepO.hpp, kernels.hip) and the ensemble (ensemble.hip)
// share: the per-cell update, the lane moves and pair stores, the argument blocks of the fused sweep, the march of
// the overlapped-strip sweep with its bodies (sweepO_march), the ghost-fill rule.  No
// kernel and no launcher is defined here.  The geometry of a strip (OverlapGeom), the rule of SPECIALISE_EDGES and the
// Tiling inside SweepArgs are sweep_plan.hpp's (host arithmetic, through internal.hpp): here they are compile-time
// constants and an argument the kernel decodes.
//
// The path is HBM-bandwidth-bound by nature (16 algorithmic bytes and 12-15 fp64 operations per cell
// update: 15 in the reference's sequence, 14 with E - 2c fused, 12 for power-of-two velocities), so there is no MFMA here.  What matters:
//   * 16-byte-per-lane coalesced row accesses on 128-byte-aligned rows, each cell read once and
//     written once per PASS: vertical reuse in registers while a wavefront marches up its column
//     strip, horizontal reuse through cross-lane DPP moves (an LDS-staged variant is kept for
//     comparison), row loads kept in flight to cover HBM latency, XCD-aware block->tile map;
//   * temporal blocking: up to seven time levels stay in registers per pass (k_sweepO_dpp, the
//     default), which divides the HBM traffic per step by as much and leaves the kernel bound by the
//     reference's own fp64 add/mul stream.
//
// Arithmetic follows the reference's association order exactly (reference
// src/diffusion.cpp:9-16, src/advection.cpp:13-33) and every unit that includes this file is compiled with
// -ffp-contract=off, so every kernel is bit-identical to the reference CPU path.
#pragma once
#include <algorithm>
#include <type_traits>

#include "internal.hpp"

#pragma clang fp contract(off)

namespace csim {

// -------------------------------------------------------------------------------------------
// per-cell update:  o = c + (dt*D)*lap;  o = o + (-dt)*(vx*dudx + vy*dudy)
//   lap  = ((E - 2c) + W)/(dx*dx) + ((N - 2c) + S)/(dy*dy)
//   dudx = vx >= 0 ? (c - W)/dx : (E - c)/dx      (dudy likewise)
// DIV 0: dx == dy == 1, x/1 == x.  DIV 1: all divisors are powers of two, so x * (1/d) is the
// correctly rounded quotient too (bit-identical to x/d).  DIV 2: true IEEE fp64 division.
// -------------------------------------------------------------------------------------------
// FAST: E - 2c as ONE operation, fma(-2, c, E).  2c is exact in binary floating point (subnormals included), so
// the fused form rounds the same real number E - 2c once, exactly like the subtraction does — unless 2c
// overflows (|c| >= 2^1023), where the reference gets +-inf and the fma a finite number.  Only k_sweepO_dpp's
// interior body uses it, under a guard that re-runs the tile with the plain form if that could happen (see
// sweepO_march); it removes one of the 15 fp64 operations per cell (P2 below: two more of the remaining 14).
template <int DIV, bool FAST = false>
__device__ __forceinline__ double diffuse_term(double c, double W, double E, double S, double N,
                                               const Phys& p) {
    double lx, ly;
    if (FAST) {
        lx = __builtin_fma(-2.0, c, E) + W;
        ly = __builtin_fma(-2.0, c, N) + S;
    } else {
        const double tc = 2.0 * c;
        lx = (E - tc) + W;
        ly = (N - tc) + S;
    }
    if (DIV == 1) {
        lx = lx * p.rdx2;
        ly = ly * p.rdy2;
    } else if (DIV == 2) {
        lx = lx / p.dx2;
        ly = ly / p.dy2;
    }
    const double lap = lx + ly;
    return c + p.kdiff * lap;
}

// SX / SY: upwind direction known at compile time (1: v >= 0, 0: v < 0, -1: decided at run
// time).  The compute-bound multi-step kernels are instantiated per sign so that neither both
// differences nor a per-lane select are evaluated.
template <int DIV, int SX = -1, int SY = -1>
__device__ __forceinline__ double advect_term(double c, double W, double E, double S, double N,
                                              const Phys& p) {
    double gx, gy;
    if (SX == 1)
        gx = c - W;
    else if (SX == 0)
        gx = E - c;
    else
        gx = (p.vx >= 0.0) ? (c - W) : (E - c);
    if (SY == 1)
        gy = c - S;
    else if (SY == 0)
        gy = N - c;
    else
        gy = (p.vy >= 0.0) ? (c - S) : (N - c);
    if (DIV == 1) {
        gx = gx * p.rdx;
        gy = gy * p.rdy;
    } else if (DIV == 2) {
        gx = gx / p.dx;
        gy = gy / p.dy;
    }
    const double adv = p.vx * gx + p.vy * gy;
    return p.mdt * adv;
}

// DIV 3 — option "contract" (opt-in, NOT bit-identical): the same update written as the 5-point stencil
// it is, a0 c + aW W + aE E + aS S + aN N with host-made coefficients (make_phys), evaluated as one
// multiply and four FMAs instead of 15 non-FMA operations.  Differs from the reference's rounding by a
// few ulp per step (tests: L_inf < 1e-10 after 1000 steps, the north-star tolerance).
//
// P2 — both velocities non-zero powers of two (option "pow2_v"; DIV 0 / 1, SX, SY in {0, 1}, FAST): the seven
// operations of the advection term as five.  With A = vx/dx and B = vy/dy (signed powers of two; rdx, rdy fold in on
// the host) the reference computes  fl(fl(A gx) + fl(B gy))  and then (-dt) times that.  Both products are exact, and
// scaling by a power of two commutes with rounding, so the sum is  B fl(q gx + gy)  with q = A/B, one fma, and the
// product with -dt is the one rounding of  K F,  K = (-dt) B  formed exactly on the host.  All of this holds as long as
// nothing lands in the subnormal range with bits to lose and nothing overflows: the tile's screen (sweepO_march) lets
// only values through that are exactly zero or at least p.slow_thr in magnitude, and below p.p2_hi; DESIGN.md §4
// derives the two bounds (make_phys).
// Signs of zeros: factoring out a POSITIVE velocity leaves q gx and gy with the signs of A gx and B gy, so F is the
// reference's sum down to the sign of a zero.  Hence vy is factored out where vy > 0 (SY == 1), vx where only vx is
// (SX == 1, SY == 0: F = fma(q, gy, gx), q = B/A).  Both negative (SX == SY == 0): vy is factored out all the same and
// an exactly cancelling sum or a pair of opposite zeros comes out as -0 where the reference has +0 — a zero m of the
// other sign, which changes o + m only where o is -0, and that goes back to a LOADED -0 (see SX = 2 below): this
// flavour's screen also sends tiles with a loaded -0 to the plain body, as the zero-velocity flavours' does.
template <int DIV, int SX = -1, int SY = -1, bool FAST = false, bool P2 = false>
__device__ __forceinline__ double cell(double c, double W, double E, double S, double N,
                                       const Phys& p) {
    if (DIV == 3) {
        double o = p.a0 * c;
        o = __builtin_fma(p.aW, W, o);
        o = __builtin_fma(p.aE, E, o);
        o = __builtin_fma(p.aS, S, o);
        return __builtin_fma(p.aN, N, o);
    }
    const double o = diffuse_term<DIV, FAST>(c, W, E, S, N, p);
    if (P2) {
        static_assert(!P2 || (FAST && DIV <= 1 && (SX == 0 || SX == 1) && (SY == 0 || SY == 1)), "see P2 above");
        const double gx = SX == 1 ? c - W : E - c;
        const double gy = SY == 1 ? c - S : N - c;
        const double F = (SY == 1 || SX == 0) ? __builtin_fma(p.p2_q, gx, gy) : __builtin_fma(p.p2_q, gy, gx);
        return o + p.p2_k * F;
    }
    // SX = 2 / SY = 2 — vx == 0 / vy == 0 (both: BASELINE configs[1], diffusion only; one: e.g. the reference's own
    // configs/dev.yaml, vy = 0).  The reference still evaluates o + (-dt) * (vx * dudx + vy * dudy).  With finite
    // differences a product with a zero velocity is +0 or -0; adding it to the other product changes nothing unless that
    // one is a zero too, and then only the SIGN of the zero sum; (-dt) times a zero is a zero; and o + (+-0) is o bit for
    // bit unless o is -0 — and c + k * lap can only be -0 where c itself is -0, level after level down to a LOADED -0.
    // So the screened interior body (FAST: every loaded value finite and below the threshold; here also: none of them -0)
    // leaves the operations of a zero component out (3 of 14 for one, all 7 for both); every other body of such an
    // instantiation evaluates them as v >= 0.
    if (FAST && (SX == 2 || SY == 2)) {
        if (SX == 2 && SY == 2) return o;
        double g;  // the one live component, as advect_term forms it
        if (SY == 2)
            g = SX == 1 ? c - W : E - c;
        else
            g = SY == 1 ? c - S : N - c;
        if (DIV == 1) g = g * (SY == 2 ? p.rdx : p.rdy);
        const double adv = (SY == 2 ? p.vx : p.vy) * g;
        return o + p.mdt * adv;
    }
    return o + advect_term<DIV, (SX == 2 ? 1 : SX), (SY == 2 ? 1 : SY)>(c, W, E, S, N, p);
}

// ---- cross-lane neighbour moves (DPP, no LDS traffic) ---------------------------------------
// wave_shr:1  lane i <- lane i-1, lane 0 keeps `edge`;  wave_shl:1  lane i <- lane i+1, lane 63
// keeps `edge` (bound_ctrl off: lanes without a source keep the old value).
__device__ __forceinline__ double from_prev_lane(double src, double edge) {
    int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(src), 0x138, 0xf, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(src), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double from_next_lane(double src, double edge) {
    int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(src), 0x130, 0xf, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(src), 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// Blocks b and b+8 share an XCD (round-robin dispatch), so give every XCD one contiguous run of
// tile ids: x-adjacent strips and y-adjacent chunks then hit the same 4 MiB L2.  Bijective for
// any grid size.  Placement only affects speed, never results.
__device__ __forceinline__ int xcd_remap(int b, int nb, int enable) {
    if (!enable || nb < 16) return b;
    const int per = nb >> 3, rem = nb & 7;
    const int xcd = b & 7, q = b >> 3;
    return xcd < rem ? xcd * (per + 1) + q : rem * (per + 1) + (xcd - rem) * per + q;
}

// write-through flavour (agent-scope relaxed atomic stores, `global_store ... sc1`): the values are in
// memory, visible to every XCD, once the wavefront's s_waitcnt vmcnt(0) returns — no L2 write-back
// (buffer_wbl2) needed.  Used by the frame tiles of a merged launch, whose outputs later kernels on
// another stream read while this kernel is still running.
__device__ __forceinline__ void store_pair_wt(double* dst, double ox, double oy, int nvalid) {
    if (nvalid >= 1)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(dst), static_cast<unsigned long long>(__double_as_longlong(ox)),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nvalid >= 2)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(dst + 1), static_cast<unsigned long long>(__double_as_longlong(oy)),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void store_pair(double* dst, double ox, double oy, int nvalid) {
    if (nvalid >= 2) {
        *reinterpret_cast<double2*>(dst) = make_double2(ox, oy);
    } else if (nvalid == 1) {
        dst[0] = ox;
    }
}

// kind[s] of a fused pass: CSIM_BC_* on physical sides, 3 where the side has a neighbour rank
// (plain stencil on the stored deep halo)
struct Bc2 {
    int kind[4];  // per side: CSIM_BC_* or 3 (= not a physical edge)
    double value;
};

// -------------------------------------------------------------------------------------------
// VAR_OVERLAP — T time steps per pass with OVERLAPPED strips (the default multi-step kernel).
// A wavefront loads 128 consecutive columns (2 per lane, 16-byte aligned) but only the inner
// 128 - 2*TP of them (TP = T rounded up to even) are its outputs: level l is valid on local
// columns [l, 127 - l], so no extra-column bookkeeping is needed at all — the W/E neighbours are
// plain DPP lane shifts (the invalid outermost lanes simply compute don't-care values) and the
// strips overlap by 2*TP columns (6 % redundant work at T = 4) instead of paying one extra
// wave-wide cell update per level (50 %).  A row of a level is ONE double2 per lane, so the whole
// T-level pipeline fits in ~107 VGPRs at T = 6.
//   - level l+1 of row r needs level l of rows r-1..r+1: the march starts T-1 rows below the chunk
//     and ends T-1 rows above it (the device layout keeps GHOST_EXTRA extra ghost rows/columns);
//   - where a strip/chunk touches a PHYSICAL edge, the ghost value of an intermediate level is not a
//     stencil result but the boundary rule applied to that level (reference src/boundary.cpp:23-53
//     run at the start of the next step): Dirichlet -> value, Neumann -> adjacent interior of the
//     same level, Periodic (no-op) -> the stored ghost, unchanged.  kind 3 = the side
//     has a neighbour rank: plain stencil on the stored deep halo.
// Ghost COLUMNS are ordinary lanes here, patched by the boundary rule on wavefronts that contain a
// physical edge.  Any nx works.
// -------------------------------------------------------------------------------------------
__device__ __forceinline__ double shift_from_prev(double src) {  // lane i <- lane i-1 (lane 0: 0)
    int lo = __builtin_amdgcn_update_dpp(0, __double2loint(src), 0x138, 0xf, 0xf, true);
    int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(src), 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shift_from_next(double src) {  // lane i <- lane i+1 (lane 63: 0)
    int lo = __builtin_amdgcn_update_dpp(0, __double2loint(src), 0x130, 0xf, 0xf, true);
    int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(src), 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// An empty volatile asm cannot be speculated, so the block it sits in stays a real (wave-uniform)
// branch instead of being if-converted into per-lane selects on the hot path.
__device__ __forceinline__ void keep_branch() { asm volatile(""); }

// Last pass of a run: the kernel also leaves, per side, the line of level T-1 (the state before
// the last step) that the reference's final halo exchange + apply_boundary would have read, so
// that the ghost ring of the result can be made exactly the reference's without a trailing
// single-step pass.  Physical side: the adjacent interior line (column 1 / nx, row 1 / ny);
// neighbour side: the ghost line itself (column 0 / nx+1, row 0 / ny+1), which this rank computes
// anyway from the deep faces — bitwise what the neighbour holds there.
struct FinLines {
    double* line[4];  // left/right: ny entries; bottom/top: nx entries; all nullptr = off
};

// The by-value argument block of k_sweepO_dpp (behind the two field pointers, which stay direct __restrict__
// parameters).  Everything a wavefront needs BEFORE or DURING its march is read from the parameter as usual; what it
// needs only rarely or only AFTER the march — the FinLines pointers, the whole FrameSync — is read from the
// kernel-argument segment at the point of use (LateArgs), so that those ~40 scalars are not kept alive (and
// spilled to VGPR lanes: 101 SGPR spills, 524 v_readlane/v_writelane per edge group of six in round 2) across the
// loop that is the kernel.
struct SweepArgs {
    int nx, ny, pitch, nstrips, swz;
    Tiling tl;
    Phys p;
    Bc2 bc;
    const unsigned* lease;  // the stepper's verdict word (M_LEASED below), nullptr where no lease machinery applies
    FinLines fin;
    FrameSync fs;
};
constexpr int SWEEP_ARGS_KERNARG_OFFSET = 16;  // two pointers precede it; alignof(SweepArgs) == 8
static_assert(alignof(SweepArgs) <= 8 && 2 * sizeof(void*) == SWEEP_ARGS_KERNARG_OFFSET,
              "LateArgs reads SweepArgs from the kernel-argument segment right behind the two field pointers");

struct LateArgs {
    typedef const SweepArgs __attribute__((address_space(4))) * Ptr;
    Ptr a;
    __device__ __forceinline__ static LateArgs get() {
        typedef const char __attribute__((address_space(4))) * Bytes;
        LateArgs l;
        l.a = (Ptr)((Bytes)__builtin_amdgcn_kernarg_segment_ptr() + SWEEP_ARGS_KERNARG_OFFSET);
        return l;
    }
    // an opaque copy of the pointer: the loads through it stay where they are written (the scalar data cache
    // serves them; the kernel-argument segment is a few hundred bytes)
    __device__ __forceinline__ Ptr here() const {
        Ptr q = a;
        asm volatile("" : "+s"(q));
        return q;
    }
    __device__ __forceinline__ double* fin_line(int side) const { return here()->fin.line[side]; }
};

template <int T, int NC = 2>
struct OverlapGeom {
    static constexpr int TP = strip_overlap(T);         // T rounded up to even
    static constexpr int STRIDE = strip_stride(T, NC);  // output columns per wavefront
};

// One row of one level in a lane: NC consecutive columns as NC / 2 aligned pairs.  NC = 2 is the strip every body was
// written for; NC = 4 is the WIDE strip of the unscreened interior bodies (sweepO_march).
template <int NC>
struct LaneRow {
    static_assert(NC == 2 || NC == 4, "columns per lane");
    double2 h[NC / 2];
    __device__ __forceinline__ double col(int q) const { return (q & 1) ? h[q >> 1].y : h[q >> 1].x; }
    __device__ __forceinline__ void set(int q, double v) {
        if (q & 1)
            h[q >> 1].y = v;
        else
            h[q >> 1].x = v;
    }
};

// FAST (interior body only): the cell update with E - 2c, N - 2c fused (diffuse_term<., true>), bit-identical to
// the plain form as long as no 2c overflows.  Guard: every value the tile loads is compared with p.fast_thr =
// 2^1022 / g^MAX_FUSE, g = the host's bound on the growth of max|u| per step; below it no level of the pass can
// reach 2^1023.  The march returns true if any lane saw a value that is not below the threshold (NaN and Inf
// included) and the caller then repeats the tile with the plain form — same loads, same stores, the reference's
// own operations.  Cost: two compares per lane and loaded row against 2 T multiplies saved.
//
// The EDGE bodies (wavefronts whose strip or chunk touches a physical edge, and the frame tiles of a final pass) are
// the interior body plus PATCHES that put the boundary rule where a level's ghost cells come out.  In the GENERIC
// flavour (M_GENERIC below; the straight-line flavours 0..6 compile their one patch in) every patch sits
// in a wave-uniform branch and works on values made opaque INSIDE that branch (pin / pin2: an empty asm the value
// passes through), so that the compiler can neither hoist the patch's moves, lane shifts and selects out of the
// branch nor turn the branch into per-lane selects executed by every level-row — which is what it did to the
// plain `if` blocks of round 2: 667 v_cndmask + 312 DPP moves + 524 v_readlane/v_writelane (101 spilled scalars)
// per group of six at T = 7, 2.2 x the instructions of the interior body.  What remains in the steady state:
//   * ghost COLUMNS (first / last strips): per level-row and side one per-lane select (Dirichlet / Periodic: the
//     ghost keeps its value; 2 v_cndmask) or a lane shift + select (Neumann; 2 DPP + 2 v_cndmask);
//   * ghost ROWS (physical bottom / top) only come out in the first ~2T and the last ~2T iterations of a chunk that
//     reaches the edge: the row tests run only in groups of six that can contain one (`rows_here`), elsewhere a
//     level-row pays one scalar branch;
//   * the FinLines emission of a run's last pass: scalar tests at level T-1, with the four line pointers read from
//     the kernel-argument segment where they are used (LateArgs) instead of living in scalars across the march.
__device__ __forceinline__ void pin(double& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin2(double2& v) { asm volatile("" : "+v"(v.x), "+v"(v.y)); }

// MODE: which body this instantiation is — ONE march loop each, so that every flavour is register-allocated like the
// interior body (several bodies chained in one function grew the kernel from 124 to 179-194 VGPRs, i.e. from 4 to 2
// wavefronts per SIMD for EVERY tile):
//   M_FAST / M_PLAIN  interior body with / without the fused E - 2c (see FAST above)
//   M_FAST_P2         M_FAST with the five-operation advection term of power-of-two velocities (cell, P2) and its
//                     wider screen; compiled where P2_BODY says so, tried first where the host enabled it (p.slow_thr > 0)
//   M_LEASED /        M_FAST / M_FAST_P2 with the screen compiled out: what the screen asks of every loaded value the
//   M_LEASED_P2       stepper has checked for the whole field, once, and holds as a lease over the steps for which the
//                     answer provably persists (the verdict word, SweepArgs::lease; bounds: lease_bounds in api.cpp,
//                     DESIGN.md §4).  They never ask for a repeat.  Compiled where LEASE_BODY / LEASE_P2_BODY say so
//   M_GENERIC         edge body with every patch behind run-time tests: tiles that can produce ghost ROWS of a
//                     physical edge (the launcher keeps them thin: bottom / top bands) and strips that hold BOTH ghost
//                     columns; also every edge tile of the instantiations that are not specialised (SPECIALISE_EDGES)
//   0..6              edge body of a strip with at most ONE ghost column and no ghost rows, its patch compiled in,
//                     straight-line like the interior body: 0 none (a final pass's frame tile that only emits
//                     FinLines), 1 / 2 left ghost kept / Neumann, 3 / 4 right ghost kept in .x / .y, 5 / 6 right
//                     ghost Neumann in .x / .y
constexpr int M_LEASED_P2 = -6, M_LEASED = -5, M_FAST_P2 = -4, M_FAST = -3, M_PLAIN = -2, M_GENERIC = -1;
constexpr unsigned LEASE_FAST = 1u, LEASE_P2 = 2u;  // bits of the verdict word: what M_FAST's / M_FAST_P2's screen asks holds field-wide

// NC: columns per lane.  Every body exists with NC = 2; the bodies without a screen and without patches (M_LEASED_P2,
// M_LEASED, M_PLAIN) also with NC = 4, for tiles whose 256 loaded columns and whose rows of every level are interior
// cells (the WIDE regions of sweep_plan.cpp).  A lane imports two doubles per level-row whatever NC is — W of its first
// column from the previous lane's last, E of its last column from the next lane's first — and a strip loses 2 TP
// columns whatever its width: with four columns per lane the same 4 DPP moves and the same 16 lost columns are paid
// for 256 columns instead of 128.  The in-lane neighbours are plain registers.
template <int DIV, int T, int MODE, int SX, int SY, int NC = 2>
__device__ __forceinline__ bool sweepO_march(const double* __restrict__ in, double* __restrict__ out,
                                             int nx, int ny, int pitch, int jb, int je, int g0, int lane,
                                             int kl, int kr, const Phys& p, int kb, int kt,
                                             LateArgs late, bool fin_any, bool fin_l, bool fin_r, bool wt) {
    constexpr int TP = OverlapGeom<T, NC>::TP;
    constexpr int STRIDE = OverlapGeom<T, NC>::STRIDE;
    constexpr bool EDGE = MODE >= M_GENERIC, P2 = MODE == M_FAST_P2 || MODE == M_LEASED_P2, GENERIC = MODE == M_GENERIC;
    constexpr bool FAST = MODE == M_FAST || MODE == M_LEASED || P2, SCREEN = MODE == M_FAST || MODE == M_FAST_P2;
    constexpr int CASE = MODE;
    static_assert(NC == 2 || (!EDGE && !SCREEN), "four columns per lane: interior bodies without a screen only");
    using Row = LaneRow<NC>;
    // this lane's first two columns, 0-based interior index (-1 = left ghost, nx = right ghost)
    const int gx = g0 + NC * lane, gy = gx + 1;
    const ptrdiff_t xoff = LPAD + gx;
    // kb / kt: kind of the bottom / top side, 3 = neighbour rank: plain stencil
    // output lanes: local columns [TP, TP + STRIDE), clipped to the interior
    const bool out_lane = NC * lane >= TP && NC * lane < TP + STRIDE && gx < nx;
    const int nvalid = nx - gx;
    // NC = 4: the lane's second pair.  TP is even, so a pair is an output as a whole; at TP = 6 the first and the last
    // output lane store one pair, at TP = 8 and TP = 4 every output lane stores both.  No clipping to nx: see above
    const bool out_pair1 = NC == 4 && NC * lane + 2 >= TP && NC * lane + 2 < TP + STRIDE;
    // lanes that hold a ghost column of a physical edge (EDGE bodies only).  g0 is even, so the right ghost column
    // (index nx) is the .x of its lane when nx is even and the .y when nx is odd: wave-uniform
    const bool ghost_ly = kl != 3 && gy == -1;
    const bool ghost_rx = kr != 3 && gx == nx, ghost_ry = kr != 3 && gy == nx;
    const bool right_in_x = (nx & 1) == 0;
    const bool ghost_cols = kl != 3 || kr != 3;  // wave-uniform

    auto load = [&](int j) {
        Row r;
#pragma unroll
        for (int h = 0; h < NC / 2; ++h)
            r.h[h] = *reinterpret_cast<const double2*>(in + static_cast<ptrdiff_t>(j) * pitch + xoff + 2 * h);
        return r;
    };

    const int r_first = jb - (T - 1);
    const int niter = (je - jb + 1) + 2 * (T - 1);
    const int last_row = r_first + niter;
    // Every load below is unconditional (row index clamped to the last row the chunk needs) and
    // the march runs whole groups of six iterations without a per-iteration exit test: a memory
    // operation that may or may not have been issued makes the compiler wait for ALL of them
    // (s_waitcnt vmcnt(0)) at the top of every iteration, which would serialise the row prefetch.
    // The <= 5 surplus iterations of a chunk whose niter is not a multiple of six compute rows
    // beyond je that are never stored (the host picks ry so that only a ragged last chunk has any).
    Row L0[6];
    Row L[T][3];
#pragma unroll
    for (int q = 0; q < 6; ++q) L0[q] = load(min(r_first - 1 + q, last_row));
    bool big = false;  // SCREEN: some loaded value is not below the threshold
    auto screen = [&](const double2& v) {
        big |= !(__builtin_fabs(v.x) < (P2 ? p.p2_hi : p.fast_thr));
        big |= !(__builtin_fabs(v.y) < (P2 ? p.p2_hi : p.fast_thr));
        if (P2) {  // exactly zero, or large enough that no level of the pass loses bits to the subnormal range (cell, P2)
            big |= __builtin_fabs(v.x) < p.slow_thr && v.x != 0.0;
            big |= __builtin_fabs(v.y) < p.slow_thr && v.y != 0.0;
        }
        if (SX == 2 || SY == 2 || (P2 && SX == 0 && SY == 0)) {  // flavours without (part of) the advection term (see cell): a loaded -0 sends the tile to the plain body too
            big |= __builtin_amdgcn_class(v.x, 0x20);
            big |= __builtin_amdgcn_class(v.y, 0x20);
        }
    };
    if (SCREEN) {  // every later row is screened when it is the `n` of level 1
        screen(L0[0].h[0]);
        screen(L0[1].h[0]);
    }
#pragma unroll
    for (int l = 0; l < T; ++l)
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int h = 0; h < NC / 2; ++h) L[l][q].h[h] = make_double2(0.0, 0.0);

    // One group = six iterations.  Level l has nothing valid to produce before iteration 2 (l - 1)
    // (its first needed row, jb - (T - l), comes out exactly then), so the first two groups are
    // separate copies of the body in which the not-yet-started levels are left out at compile time:
    // 30 of the 6 (ry + 10) level-rows of a chunk at T = 6.  (The edge body keeps the single generic
    // copy: it is rare and its code is three times the size.)
    auto group = [&](auto gtag, int k0) {
        constexpr int G = decltype(gtag)::value;
        // GENERIC: can this group of six contain a ghost row of a physical edge?  Level l = 1..T-1 produces ghost row 0
        // at iteration l + T - 2 - jb (patched from row 1 one iteration later) and ghost row ny+1 at iteration
        // ny + l + T - 1 - jb: only in groups with  k0 <= 2T - 2 - jb  (bottom)  or  k0 + 5 >= ny + T - jb  (top)
        const bool rows_here = GENERIC && ((kb != 3 && k0 <= 2 * T - 2 - jb) || (kt != 3 && k0 + 5 >= ny + T - jb));
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            {
                const int r = r_first + k0 + u;
#pragma unroll
                for (int l = 1; l <= T; ++l) {
                    if (G < 2 && 6 * G + u < 2 * (l - 1)) continue;  // compile-time: level not started yet
                    const int rho = r - l + 1;
                    const Row sr = (l == 1) ? L0[u % 6] : L[l - 1][(u + 1) % 3];
                    const Row cr = (l == 1) ? L0[(u + 1) % 6] : L[l - 1][(u + 2) % 3];
                    const Row nr = (l == 1) ? L0[(u + 2) % 6] : L[l - 1][u % 3];
                    // The stencil is evaluated on every lane and row (branch-free, the same code as
                    // the interior body); where the result is a ghost cell of a physical edge it is
                    // then replaced by the boundary rule.
                    Row orow;
                    {
                        const double Wx = shift_from_prev(cr.col(NC - 1));
                        const double Ey = shift_from_next(cr.col(0));
#pragma unroll
                        for (int q = 0; q < NC; ++q)
                            orow.set(q, cell<DIV, SX, SY, FAST, P2>(cr.col(q), q == 0 ? Wx : cr.col(q - 1), q == NC - 1 ? Ey : cr.col(q + 1),
                                                                    sr.col(q), nr.col(q), p));
                        if (SCREEN && l == 1) screen(nr.h[0]);
                    }
                    // the patches below, the FinLines and the write-through stores are the narrow strip's (EDGE bodies and
                    // frame tiles: NC = 2): they work on the row's one pair
                    const double2 c = cr.h[0];
                    double2 o = orow.h[0];
                    if (EDGE && !GENERIC && l < T) {  // the strip's one ghost column, unconditionally
                        if (CASE == 1) o.y = ghost_ly ? c.y : o.y;
                        if (CASE == 2) {
                            const double nb = shift_from_next(o.x);
                            o.y = ghost_ly ? nb : o.y;
                        }
                        if (CASE == 3) o.x = ghost_rx ? c.x : o.x;
                        if (CASE == 4) o.y = ghost_ry ? c.y : o.y;
                        if (CASE == 5) {
                            const double pb = shift_from_prev(o.y);
                            o.x = ghost_rx ? pb : o.x;
                        }
                        if (CASE == 6) o.y = ghost_ry ? o.x : o.y;
                    }
                    if (GENERIC && l < T) {
                        bool ghost_row = false;
                        if (rows_here) {
                            const bool gb = rho == 0 && kb != 3, gt = rho == ny + 1 && kt != 3;
                            ghost_row = gb || gt;
                            if (ghost_row) {  // ghost ROW of this level
                                const int kk = gb ? kb : kt;
                                if (kk != CSIM_BC_NEUMANN) {  // Dirichlet / Periodic ghosts keep their level-0 value (bc.value / stored)
                                    double2 t = c;
                                    pin2(t);
                                    o = t;
                                } else if (gt) {  // Neumann top: row ny of this level
                                    double2 t = L[l][(u + 2) % 3].h[0];
                                    pin2(t);
                                    o = t;
                                }
                                // (Neumann bottom: patched below as soon as row 1 of this level exists)
                            }
                        }
                        if (!ghost_row && ghost_cols) {  // ghost COLUMNS of this level (first / last strip)
                            if (kl == CSIM_BC_NEUMANN) {  // left ghost (.y of its lane) := column 0 (.x of the next lane)
                                double t = o.x;
                                pin(t);
                                const double nb = shift_from_next(t);
                                o.y = ghost_ly ? nb : o.y;
                            } else if (kl != 3) {  // Dirichlet / Periodic: unchanged through the levels
                                double t = c.y;
                                pin(t);
                                o.y = ghost_ly ? t : o.y;
                            }
                            if (kr == CSIM_BC_NEUMANN) {  // right ghost := column nx-1 (.y of the previous lane, or the lane's own .x)
                                if (right_in_x) {
                                    double t = o.y;
                                    pin(t);
                                    const double pb = shift_from_prev(t);
                                    o.x = ghost_rx ? pb : o.x;
                                } else {
                                    double t = o.x;
                                    pin(t);
                                    o.y = ghost_ry ? t : o.y;
                                }
                            } else if (kr != 3) {
                                if (right_in_x) {
                                    double t = c.x;
                                    pin(t);
                                    o.x = ghost_rx ? t : o.x;
                                } else {
                                    double t = c.y;
                                    pin(t);
                                    o.y = ghost_ry ? t : o.y;
                                }
                            }
                        }
                    }
                    if (EDGE && T >= 2 && l == T - 1 && fin_any) {  // see FinLines
                        keep_branch();
                        if (rho >= jb && rho <= je) {
                            if (fin_l && (kl != 3 ? gx == 0 : gy == -1)) late.fin_line(CSIM_LEFT)[rho - 1] = kl != 3 ? o.x : o.y;
                            if (fin_r) {
                                const int col = kr != 3 ? nx - 1 : nx;
                                if (gx == col) late.fin_line(CSIM_RIGHT)[rho - 1] = o.x;
                                if (gy == col) late.fin_line(CSIM_RIGHT)[rho - 1] = o.y;
                            }
                        }
                        if (jb == 1 && rho == (kb != 3 ? 1 : 0) && out_lane) store_pair(late.fin_line(CSIM_BOTTOM) + gx, o.x, o.y, nvalid);
                        if (je == ny && rho == (kt != 3 ? ny : ny + 1) && out_lane) store_pair(late.fin_line(CSIM_TOP) + gx, o.x, o.y, nvalid);
                    }
                    if (l < T) {
                        if (GENERIC && rows_here && rho == 1 && kb == CSIM_BC_NEUMANN) {  // ghost row 0 := row 1
                            double2 t = o;
                            pin2(t);
                            L[l][(u + 2) % 3].h[0] = t;
                        }
                        if (NC == 2) orow.h[0] = o;
                        L[l][u % 3] = orow;
                    } else if (NC == 4) {  // whole pairs, never clipped
                        if (rho >= jb && rho <= je) {
                            double* dst = out + static_cast<ptrdiff_t>(rho) * pitch + xoff;
                            if (out_lane) *reinterpret_cast<double2*>(dst) = orow.h[0];
                            if (out_pair1) *reinterpret_cast<double2*>(dst + 2) = orow.h[NC / 2 - 1];
                        }
                    } else if (rho >= jb && rho <= je && out_lane) {
                        if (wt) {  // wave-uniform: frame tile of a merged launch
                            keep_branch();
                            store_pair_wt(out + static_cast<ptrdiff_t>(rho) * pitch + xoff, o.x, o.y, nvalid);
                        } else {
                            store_pair(out + static_cast<ptrdiff_t>(rho) * pitch + xoff, o.x, o.y, nvalid);
                        }
                    }
                }
                L0[u % 6] = load(min(r + 5, last_row));  // row r-1 is dead: its slot takes row r+5
            }
        }
    };
    using G2 = std::integral_constant<int, 2>;
    if (EDGE) {
        for (int k0 = 0; k0 < niter; k0 += 6) group(G2{}, k0);
    } else {
        group(std::integral_constant<int, 0>{}, 0);
        if (niter > 6) group(std::integral_constant<int, 1>{}, 6);
        for (int k0 = 12; k0 < niter; k0 += 6) group(G2{}, k0);
    }
    return SCREEN && __builtin_amdgcn_ballot_w64(big) != 0;
}

// Which instantiations get the straight-line edge flavours: the rule is specialise_edges (sweep_plan.hpp), which the
// tile plan reads too.
template <int DIV, int T>
struct SPECIALISE_EDGES {
    static constexpr bool value = specialise_edges(DIV, T);
};

// Which instantiations of k_sweepO_dpp carry the M_FAST_P2 body: the same arithmetic modes and depths, with both
// velocity components non-zero.  Elsewhere (and in the ensemble's kernel) p.slow_thr is ignored.
template <int DIV, int T, int SX, int SY>
struct P2_BODY {
    static constexpr bool value = SPECIALISE_EDGES<DIV, T>::value && (SX == 0 || SX == 1) && (SY == 0 || SY == 1);
};

// Which carry the unscreened bodies: M_LEASED wherever M_FAST is the whole screen (both velocity components non-zero;
// the zero-velocity flavours also screen for a loaded -0 and keep their screened body), M_LEASED_P2 wherever M_FAST_P2
// is, except SX = SY = 0, whose screen has the -0 test too.
template <int DIV, int T, int SX, int SY>
struct LEASE_BODY {
    static constexpr bool value = P2_BODY<DIV, T, SX, SY>::value;
};
template <int DIV, int T, int SX, int SY>
struct LEASE_P2_BODY {
    static constexpr bool value = P2_BODY<DIV, T, SX, SY>::value && !(SX == 0 && SY == 0);
};

// -------------------------------------------------------------------------------------------
// Ghost fill = unpack of the staged neighbour halos (reference src/halo.cpp:28-43) followed by
// apply_boundary (reference src/boundary.cpp:12-54) in ONE launch, written to the current
// field and, when `b` is given, identically to the ping-pong partner so that after the sweep
// and swap the new field carries the same ghost ring the reference gets from its copy
// (src/main.cpp:104) + ring copy (src/diffusion.cpp:18-25).
// The reference fills sides sequentially (left, right, bottom, top), which only matters at the
// four corners; they are evaluated functionally by one thread from values no other thread of
// this launch writes.
// -------------------------------------------------------------------------------------------
struct GhostDev {
    int bc[4];
    int phys[4];
    double value;
    const double* recv[4];
    const double* adj[4];  // != nullptr: the adjacent interior line of that side is read from here, not from `a`
    int ext_depth;  // > 0: also continue physical edges over that many halo cells (see ghost_extend_cell)
};

__device__ __forceinline__ size_t at(int i, int j, int pitch) {
    return static_cast<size_t>(j) * pitch + (LPAD - 1) + i;
}

// One thread's share of a ghost fill (k_ghost_fill, and k_ensemble_ghost in ensemble.hip): t < ny the two ghost
// columns of row t + 1, t < nx the two ghost rows of column t + 1, t == max(nx, ny) the four corners.
__device__ __forceinline__ void ghost_fill_cell(double* __restrict__ a, double* __restrict__ b, int nx, int ny,
                                                int pitch, const GhostDev& g, int t) {
    auto put = [&](size_t o, double v) {
        a[o] = v;
        if (b) b[o] = v;
    };
    if (t < ny) {  // ghost columns at row j = t + 1
        const int j = t + 1;
        for (int s = CSIM_LEFT; s <= CSIM_RIGHT; ++s) {
            const int ig = s == CSIM_LEFT ? 0 : nx + 1;
            const int ia = s == CSIM_LEFT ? 1 : nx;
            if (g.phys[s]) {
                if (g.bc[s] == CSIM_BC_DIRICHLET)
                    put(at(ig, j, pitch), g.value);
                else if (g.bc[s] == CSIM_BC_NEUMANN)
                    put(at(ig, j, pitch), g.adj[s] ? g.adj[s][t] : a[at(ia, j, pitch)]);
            } else if (g.recv[s]) {
                put(at(ig, j, pitch), g.recv[s][t]);
            }
        }
    }
    if (t < nx) {  // ghost rows at column i = t + 1
        const int i = t + 1;
        for (int s = CSIM_BOTTOM; s <= CSIM_TOP; ++s) {
            const int jg = s == CSIM_BOTTOM ? 0 : ny + 1;
            const int ja = s == CSIM_BOTTOM ? 1 : ny;
            if (g.phys[s]) {
                if (g.bc[s] == CSIM_BC_DIRICHLET)
                    put(at(i, jg, pitch), g.value);
                else if (g.bc[s] == CSIM_BC_NEUMANN)
                    put(at(i, jg, pitch), g.adj[s] ? g.adj[s][t] : a[at(i, ja, pitch)]);
            } else if (g.recv[s]) {
                put(at(i, jg, pitch), g.recv[s][t]);
            }
        }
    }
    const int tc = nx > ny ? nx : ny;
    if (t == tc) {  // the four corners
        for (int cs = CSIM_LEFT; cs <= CSIM_RIGHT; ++cs) {
            const int ig = cs == CSIM_LEFT ? 0 : nx + 1;
            const int ia = cs == CSIM_LEFT ? 1 : nx;
            for (int rs = CSIM_BOTTOM; rs <= CSIM_TOP; ++rs) {
                const int jg = rs == CSIM_BOTTOM ? 0 : ny + 1;
                const int ja = rs == CSIM_BOTTOM ? 1 : ny;
                const bool row_d = g.phys[rs] && g.bc[rs] == CSIM_BC_DIRICHLET;
                const bool row_n = g.phys[rs] && g.bc[rs] == CSIM_BC_NEUMANN;
                const bool col_d = g.phys[cs] && g.bc[cs] == CSIM_BC_DIRICHLET;
                const bool col_n = g.phys[cs] && g.bc[cs] == CSIM_BC_NEUMANN;
                if (row_d) {
                    put(at(ig, jg, pitch), g.value);
                } else if (row_n) {
                    // row rule copies the already column-filled ghost cell (ig, ja)
                    double v;
                    if (col_d)
                        v = g.value;
                    else if (col_n)
                        v = g.adj[cs] ? g.adj[cs][ja - 1] : a[at(ia, ja, pitch)];
                    else if (!g.phys[cs] && g.recv[cs])
                        v = g.recv[cs][ja - 1];
                    else
                        v = a[at(ig, ja, pitch)];
                    put(at(ig, jg, pitch), v);
                } else if (col_d) {
                    put(at(ig, jg, pitch), g.value);
                } else if (col_n) {
                    // column rule copies ghost-row cell (ia, jg): stable (periodic) or just received
                    double v;
                    if (!g.phys[rs] && g.recv[rs])
                        v = g.recv[rs][ia - 1];
                    else
                        v = a[at(ia, jg, pitch)];
                    put(at(ig, jg, pitch), v);
                }
            }
        }
    }
}

}  // namespace csim
