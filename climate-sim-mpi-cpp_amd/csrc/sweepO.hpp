// sweepO.hpp — k_sweepO_dpp (2-7 steps/pass, overlapped strips, the DEFAULT sweep) around the march of
// sweep_core.hpp, and its launcher templates sweepO_div / sweepO_T.  sweepO_inst.hip instantiates one depth per
// translation unit; kernels.hip only declares sweepO_T.  In file order: what the kernel alone needs (face stores,
// the CSIM_TRACE hook of tools/wavetrace.hip), the kernel, the launcher.  How a launch is cut into tiles is not
// decided here: the launcher is handed a SweepPlan (sweep_plan.cpp, host arithmetic that a CPU program checks).
#pragma once
#include "sweep_core.hpp"

#pragma clang fp contract(off)

namespace csim {

// Direct faces (merged launch): one cell (column i in 0..nx+1, row j in 0..ny+1; 0 and n+1 = ghost lines) of the
// field a frame tile has just written goes into every face of the NEXT pass it belongs to.  Indexing is
// k_halo2_pack's for depth H: column faces [c][j] over rows 0..ny+1, row faces [r][i] over columns 0..nx+1 (the
// ghost entries travel along: Periodic ghosts are never rewritten), corner blocks [r][c] of interior cells.
__device__ __forceinline__ void face_store_cell(const FrameSync& fs, int i, int j, double v, int nx, int ny) {
    const int H = fs.face_depth;
    const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(v));
    auto put = [&](double* face, int idx) {  // write-through, like the tile's own result stores
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(face + idx), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    const bool in_i = i >= 1 && i <= nx, in_j = j >= 1 && j <= ny;
    const bool l = in_i && i <= H, r = in_i && i >= nx - H + 1, b = in_j && j <= H, t = in_j && j >= ny - H + 1;
    const int cl = i - 1, cr = i - (nx - H + 1), rb = j - 1, rt = j - (ny - H + 1);
    if (l && fs.face[0]) put(fs.face[0], cl * (ny + 2) + j);
    if (r && fs.face[1]) put(fs.face[1], cr * (ny + 2) + j);
    if (b && fs.face[2]) put(fs.face[2], rb * (nx + 2) + i);
    if (t && fs.face[3]) put(fs.face[3], rt * (nx + 2) + i);
    if (l && b && fs.face[4]) put(fs.face[4], rb * H + cl);
    if (r && b && fs.face[5]) put(fs.face[5], rb * H + cr);
    if (l && t && fs.face[6]) put(fs.face[6], rt * H + cl);
    if (r && t && fs.face[7]) put(fs.face[7], rt * H + cr);
}

#ifdef CSIM_TRACE
// tools/wavetrace.hip only: start/end time (100 MHz wall clock) and placement of every wavefront
__device__ unsigned long long* g_wave_trace = nullptr;
struct WaveTrace {
    int slot, lane;
    unsigned long long t0;
    __device__ WaveTrace(int s, int l) : slot(s), lane(l), t0(wall_clock64()) {}
    __device__ ~WaveTrace() {
        if (lane == 0 && g_wave_trace) {
            g_wave_trace[3 * slot] = t0;
            g_wave_trace[3 * slot + 1] = wall_clock64();
            g_wave_trace[3 * slot + 2] = (static_cast<unsigned long long>(__builtin_amdgcn_s_getreg(63508)) << 32) |
                                         static_cast<unsigned>(__builtin_amdgcn_s_getreg(63492));
        }
    }
};
#endif

// WIDE: the instantiation that also carries the wide strips' bodies (sweepO_march, NC = 4) for the regions a wide plan
// marks (sweep_plan.cpp); it is register-allocated for those (two wavefronts per SIMD), and the narrow tiles of such a
// launch — the left and right strips, the bands — run every body below at that occupancy.  Compiled where
// WIDE_KERNEL says so; a plan without wide regions is launched with WIDE = false.
template <int DIV, int T, int SX, int SY, bool WIDE = false>
__global__ __launch_bounds__(256) void k_sweepO_dpp(const double* __restrict__ in, double* __restrict__ out, SweepArgs a) {
    constexpr int TP = OverlapGeom<T>::TP;
    constexpr int STRIDE = OverlapGeom<T>::STRIDE;
    const int nx = a.nx, ny = a.ny, pitch = a.pitch;
    const LateArgs late = LateArgs::get();
    const int lane = threadIdx.x & 63;
    // readfirstlane: tells the compiler the wave index (and the strip, edge kinds and row range
    // derived from it) is wave-uniform, so those tests become scalar branches
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef CSIM_TRACE
    WaveTrace trace_scope(blockIdx.x * 4 + wave, lane);
#endif
    // blocks [0, frame_blocks): the frame tiles in plain order; the last tail_blocks blocks: the tail tiles in
    // plain order; the blocks in between own the main tiles, XCD-remapped among themselves
    // (this decode — block -> tile -> region -> strip, jb, je — believes the plan's numbers blindly;
    // tools/sweep_plan_host_check.cpp restates it and checks on the CPU that it reaches every tile of every plan once)
    int tile;
    bool frame_tile = false;
    {
        const int b = blockIdx.x;
        if (b < a.tl.frame_blocks) {
            tile = 4 * b + wave;
            if (tile >= a.tl.frame_tiles) return;  // padding of the last frame block
            frame_tile = true;
        } else {
            const int lb = b - a.tl.frame_blocks, nb_mid = gridDim.x - a.tl.frame_blocks - a.tl.tail_blocks;
            tile = a.tl.frame_tiles + (lb < nb_mid ? xcd_remap(lb, nb_mid, a.swz) : lb) * 4 + wave;
        }
    }
    if (tile >= a.tl.ntiles) return;  // wave-uniform
    int t0 = 0, x0 = a.tl.r[0].x0, wide = a.tl.r[0].wide, nstrip = a.tl.r[0].nstrip, j0 = a.tl.r[0].j0, j1 = a.tl.r[0].j1, ry = a.tl.r[0].ry;
#pragma unroll
    for (int q = 1; q < 8; ++q)
        if (q < a.tl.nregions && tile >= a.tl.r[q - 1].t_end) {
            t0 = a.tl.r[q - 1].t_end;
            x0 = a.tl.r[q].x0, wide = a.tl.r[q].wide, nstrip = a.tl.r[q].nstrip, j0 = a.tl.r[q].j0, j1 = a.tl.r[q].j1, ry = a.tl.r[q].ry;
        }
    (void)wide;  // read by the WIDE instantiation only
    const int local = tile - t0;
    const int strip = local % nstrip;  // within its region
    const int chunk = local / nstrip;
    const int jb = j0 + chunk * ry;
    const int je = min(jb + ry - 1, j1);
    if constexpr (WIDE) {
        if (wide) {
            // A wide tile is interior by construction (sweep_plan.cpp: its 256 loaded columns are interior columns, no
            // level of it meets a ghost row, it is no frame tile), and its bodies have no screen: the verdict word picks
            // the leased 12-operation body, else the leased 14-operation one, else the reference's own sequence, which
            // needs neither a screen nor a repeat.
            const int g0w = x0 + strip * strip_stride(T, 4) - TP;
            unsigned lease = 0;
            if (a.lease != nullptr) lease = __builtin_amdgcn_readfirstlane(*a.lease);
#define CSIM_MARCH_WIDE(MODE_) \
    sweepO_march<DIV, T, MODE_, SX, SY, 4>(in, out, nx, ny, pitch, jb, je, g0w, lane, 3, 3, a.p, 3, 3, late, false, false, false, false)
            if (a.p.slow_thr > 0.0 && (lease & LEASE_P2) != 0) {
                keep_branch();
                CSIM_MARCH_WIDE(M_LEASED_P2);
            } else if (a.p.fast_thr > 0.0 && (lease & LEASE_FAST) != 0) {
                keep_branch();
                CSIM_MARCH_WIDE(M_LEASED);
            } else {
                keep_branch();
                CSIM_MARCH_WIDE(M_PLAIN);
            }
#undef CSIM_MARCH_WIDE
            return;
        }
    }
    const int g0 = x0 + strip * STRIDE - TP;
    // the first strip holds the left ghost column, the last one stores column nx - 1
    const bool first = g0 == -TP, last = g0 + TP + STRIDE >= nx;
    // a strip meets the left ghost column iff it is the first one; the right ghost column (index
    // nx) lies inside every strip whose 128 loaded columns reach it
    const int kl = first ? a.bc.kind[CSIM_LEFT] : 3;
    const int kr = g0 + WAVE_COLS > nx ? a.bc.kind[CSIM_RIGHT] : 3;
    const int kb = a.bc.kind[CSIM_BOTTOM], kt = a.bc.kind[CSIM_TOP];
    // on the last pass of a run the frame tiles also take the edge body: they emit the FinLines
    const bool fin_frame = a.fin.line[CSIM_BOTTOM] != nullptr && (first || last || jb == 1 || je == ny);
    const bool edge = kl != 3 || kr != 3 || (kb != 3 && jb - (T - 1) < 1) || (kt != 3 && je + (T - 1) > ny) || fin_frame;
    if (frame_tile && a.fs.prio) __builtin_amdgcn_s_setprio(3);  // the faces wait for these: issue ahead of the co-resident bulk
    const bool signalling = frame_tile && a.fs.flag != nullptr;  // merged launch: this wavefront counts itself below
    const bool wt = signalling && a.fs.fence == 0;
    if (edge) {
        // Edge wavefronts run a little longer than interior ones and would finish last, leaving the rest of the chip
        // idle (29 % of a 4096 x 8192 launch with round 1's edge body, tools/wavetrace.hip): give them issue priority.
        __builtin_amdgcn_s_setprio(3);
        const bool rows = (kb != 3 && jb - (T - 1) < 1) || (kt != 3 && je + (T - 1) > ny);
        int col_case = 0;
        if (kl != 3 && kr != 3)
            col_case = 7;
        else if (kl != 3)
            col_case = kl == CSIM_BC_NEUMANN ? 2 : 1;
        else if (kr != 3)
            col_case = (kr == CSIM_BC_NEUMANN ? 5 : 3) + (nx & 1);  // g0 is even: the right ghost column is a .x iff nx is even
        if (!SPECIALISE_EDGES<DIV, T>::value || rows || col_case == 7) col_case = -1;
#define CSIM_MARCH(MODE_) \
    sweepO_march<DIV, T, MODE_, SX, SY>(in, out, nx, ny, pitch, jb, je, g0, lane, kl, kr, a.p, kb, kt, late, fin_frame, first, last, wt)
        switch (col_case) {
            case 0: if (SPECIALISE_EDGES<DIV, T>::value) CSIM_MARCH(0); break;
            case 1: if (SPECIALISE_EDGES<DIV, T>::value) CSIM_MARCH(1); break;
            case 2: if (SPECIALISE_EDGES<DIV, T>::value) CSIM_MARCH(2); break;
            case 3: if (SPECIALISE_EDGES<DIV, T>::value) CSIM_MARCH(3); break;
            case 4: if (SPECIALISE_EDGES<DIV, T>::value) CSIM_MARCH(4); break;
            case 5: if (SPECIALISE_EDGES<DIV, T>::value) CSIM_MARCH(5); break;
            case 6: if (SPECIALISE_EDGES<DIV, T>::value) CSIM_MARCH(6); break;
            default: CSIM_MARCH(M_GENERIC); break;
        }
    } else {
        bool redo = true;
        if (DIV != 3 && a.p.fast_thr > 0.0) {
            // The verdict word, once per wavefront and wave-uniform (a scalar load through the kernel argument): the
            // stepper guarantees that it holds for every step of this pass (lease_for_pass, passes.cpp), so a leased
            // body needs neither the screen nor a repeat.  Leased P2, else leased FAST, else the screened chain.
            unsigned lease = 0;
            if constexpr (LEASE_BODY<DIV, T, SX, SY>::value) {
                if (a.lease != nullptr) lease = __builtin_amdgcn_readfirstlane(*a.lease);
            }
            bool leased = false;
            if constexpr (LEASE_P2_BODY<DIV, T, SX, SY>::value) {
                if (a.p.slow_thr > 0.0 && (lease & LEASE_P2) != 0) {
                    keep_branch();
                    CSIM_MARCH(M_LEASED_P2);
                    leased = true;
                }
            }
            if constexpr (LEASE_BODY<DIV, T, SX, SY>::value) {
                // (not where the host enabled the 12-operation form and only its lease was refused: the screened
                // M_FAST_P2 is still fewer instructions than the unscreened 14-operation body)
                if (!leased && (lease & LEASE_FAST) != 0 && !(a.p.slow_thr > 0.0)) {
                    keep_branch();
                    CSIM_MARCH(M_LEASED);
                    leased = true;
                }
            }
            if (leased) {
                redo = false;
            } else if constexpr (P2_BODY<DIV, T, SX, SY>::value) {
                if (a.p.slow_thr > 0.0) {
                    keep_branch();
                    redo = CSIM_MARCH(M_FAST_P2);
                } else {
                    redo = CSIM_MARCH(M_FAST);
                }
            } else {
                redo = CSIM_MARCH(M_FAST);
            }
        }
        if (redo) {
            keep_branch();
            CSIM_MARCH(M_PLAIN);
        }
    }
#undef CSIM_MARCH
    if (signalling) {
        // Merged launch: the comm stream is parked on `flag` (hipStreamWaitValue64) and goes on to pack and
        // send the next pass's faces as soon as EVERY frame tile is in memory — while this very kernel is
        // still sweeping the bulk.  The consumers are later kernels on another stream and may run on any XCD,
        // so a frame tile's outputs must be in memory, not in this XCD's write-back L2, before it counts
        // itself: its result stores are write-through (store_pair_wt) and only have to be drained here.  (An
        // agent-scope release fence, i.e. buffer_wbl2 per wavefront, also works but writes back the dirty
        // output lines of the whole bulk each time: measured +40 us per 165 us pass; kept as fence = 1.)  The
        // wavefront that completes the count re-arms the counter and publishes the pass number (system scope:
        // the waiting side reads it through the command processor).
        // Everything from here on is read from the kernel-argument segment NOW (LateArgs): nothing of FrameSync was
        // alive during the march.
        const LateArgs::Ptr ka = late.here();
        FrameSync fs;
        fs.counter = ka->fs.counter, fs.flag = ka->fs.flag, fs.pass = ka->fs.pass, fs.nframe = ka->fs.nframe;
        fs.fence = ka->fs.fence, fs.face_depth = ka->fs.face_depth;
#pragma unroll
        for (int d = 0; d < 8; ++d) fs.face[d] = ka->fs.face[d];
        if (fs.fence == 0)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (fs.fence == 0 && fs.face_depth > 0) {
            // Direct faces: this wavefront copies the part of its tile that belongs to a face of the NEXT pass
            // (and the ghost entries beside it) into the send buffers, so the comm stream can post the RCCL
            // group at the flag without a pack kernel in between.  Done after the march by reading the tile
            // back (its stores are drained and written through; the loads bypass the vector L1): the same
            // stores inside the march loop cost 20 more VGPRs, i.e. one wavefront per SIMD.
            const int H = fs.face_depth;
            const int gx = g0 + 2 * lane;
            const bool out_lane = 2 * lane >= TP && 2 * lane < TP + STRIDE && gx < nx;
            const bool rows_near = jb <= H || je >= ny - H + 1;              // wave-uniform
            const bool cols_near = g0 + TP < H || g0 + TP + STRIDE > nx - H;  // wave-uniform
            if (rows_near || cols_near) {
                const int jf0 = jb == 1 ? 0 : jb, jf1 = je == ny ? ny + 1 : je;
                auto ldf = [&](const double* q) {
                    return __longlong_as_double(static_cast<long long>(__hip_atomic_load(
                        reinterpret_cast<const unsigned long long*>(q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
                };
                for (int rho = jf0; rho <= jf1; ++rho) {
                    if (!out_lane) continue;
                    const double* src = out + static_cast<ptrdiff_t>(rho) * pitch + LPAD + gx;  // cell (gx + 1, rho)
                    face_store_cell(fs, gx + 1, rho, ldf(src), nx, ny);
                    if (gx + 1 < nx) face_store_cell(fs, gx + 2, rho, ldf(src + 1), nx, ny);
                    if (gx == 0) face_store_cell(fs, 0, rho, ldf(src - 1), nx, ny);
                    if (gx + 1 == nx) face_store_cell(fs, nx + 1, rho, ldf(src + 1), nx, ny);
                    if (gx + 2 == nx) face_store_cell(fs, nx + 1, rho, ldf(src + 2), nx, ny);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        if (fs.fence == 1) __threadfence();  // plain result stores + agent-scope fence per wavefront (measured alternative)
        // Ordering (ISA level; no C++ happens-before is claimed): every store of this wavefront that a consumer may
        // read — tile results and face copies — is an agent-scope write-through store (global_store ... sc1), and the
        // s_waitcnt vmcnt(0) above returns only once each of them has been acknowledged by memory.  The counter
        // increment below is therefore issued after the data is globally visible; it can be relaxed, because the only
        // thing ordered after it is the flag store of the LAST arriver, and that wavefront's own data was drained by
        // its own s_waitcnt before its own increment — the increments of the others precede it in the counter's
        // modification order, each issued after that wavefront's drain.  The flag itself is a system-scope release
        // store; the waiting side is the command processor (hipStreamWaitValue64), and every kernel launched behind the
        // wait begins with the usual acquire (L2 invalidate / write-back state of a kernel boundary).
        if (lane == 0) {
            const unsigned done = atomicAdd(fs.counter, 1u);
            if (done == fs.nframe - 1) {
                atomicExch(fs.counter, 0u);
                __hip_atomic_store(fs.flag, fs.pass, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// ============================================================================================
// launcher of the overlapped-strip sweep (templates: one depth per translation unit, see sweepO_inst.hip)
// ============================================================================================

// three steps: take the plan (sweep_plan.cpp: the launcher's caller built it), fill SweepArgs, dispatch on the sign class
template <int DIV, int T, bool WIDE = false>
hipError_t sweepO_div(const double* in, double* out, int pitch, const Phys& p, const SweepCfg& cfg, const Bc2& bc,
                      const FinLines& fin, const SweepPlan& plan, hipStream_t st, FrameSync fs, const unsigned* lease) {
    if (plan.empty) return hipSuccess;
    if (plan.wide != WIDE) return hipErrorInvalidValue;  // wide regions are decoded by the WIDE kernel only
    if (plan.signals)
        fs.nframe = plan.nframe;
    else
        fs = FrameSync{};
    const dim3 grid(plan.nblocks), block(256);
    SweepArgs ka;
    ka.nx = plan.nx, ka.ny = plan.ny, ka.pitch = pitch, ka.nstrips = plan.nstrips, ka.swz = cfg.xcd_swizzle;
    ka.tl = plan.tl, ka.p = p, ka.bc = bc, ka.lease = lease, ka.fin = fin, ka.fs = fs;
#define CSIM_LAUNCH_O(SXV, SYV) \
    hipLaunchKernelGGL((k_sweepO_dpp<DIV, T, SXV, SYV, WIDE>), grid, block, cfg.lds_bytes, st, in, out, ka)
#ifdef CSIM_ISA_PROBE
    CSIM_LAUNCH_O(1, 1);
#else
    if constexpr (WIDE) {  // only the flavours WIDE_KERNEL names exist: a plan asked for another one by mistake
        switch (sign_class(p)) {
            case 4: CSIM_LAUNCH_O(1, 1); break;
            case 3: CSIM_LAUNCH_O(1, 0); break;
            case 1: CSIM_LAUNCH_O(0, 1); break;
            default: return hipErrorInvalidValue;
        }
    } else if (DIV == 3) {  // coefficient form: the upwind directions are folded into the coefficients
        CSIM_LAUNCH_O(1, 1);
    } else {
        // zero velocity components (DIV 0 / 1; the IEEE-division form keeps its four sign flavours): code 2 per axis
        switch (sign_class(p)) {
            case 8: if constexpr (DIV <= 1) CSIM_LAUNCH_O(2, 2); break;
            case 7: if constexpr (DIV <= 1) CSIM_LAUNCH_O(2, 1); break;
            case 6: if constexpr (DIV <= 1) CSIM_LAUNCH_O(2, 0); break;
            case 5: if constexpr (DIV <= 1) CSIM_LAUNCH_O(1, 2); break;
            case 2: if constexpr (DIV <= 1) CSIM_LAUNCH_O(0, 2); break;
            case 4: CSIM_LAUNCH_O(1, 1); break;
            case 3: CSIM_LAUNCH_O(1, 0); break;
            case 1: CSIM_LAUNCH_O(0, 1); break;
            default: CSIM_LAUNCH_O(0, 0); break;
        }
    }
#endif
#undef CSIM_LAUNCH_O
    return hipGetLastError();
}

template <int T>
hipError_t sweepO_T(const double* in, double* out, int pitch, const Phys& p, const SweepCfg& cfg, const Bc2& bc,
                    const FinLines& fin, const SweepPlan& plan, hipStream_t st, const FrameSync& fs, const unsigned* lease) {
#ifdef CSIM_ISA_PROBE  // tools: only the instantiation bench.py runs (dx = dy = 1, vx, vy >= 0), for a readable listing
    // the plan took its edge rule from p.div_mode (plan_sweepO): a probe build run with another mode would pair a plan
    // without bands with a kernel that specialises its edges
    if (p.div_mode != 0) return hipErrorInvalidValue;
    return sweepO_div<0, T>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
#else
    switch (p.div_mode) {
        case 0: return sweepO_div<0, T>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
        case 1: return sweepO_div<1, T>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
        case 3: return sweepO_div<3, T>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
        default: return sweepO_div<2, T>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
    }
#endif
}

// the same for a plan with wide regions: depths 6 and 7, DIV 0 / 1 (wide_strips_compiled), both velocities non-zero and
// not both negative (LEASE_P2_BODY) — anything else is an error, never another kernel
template <int T>
hipError_t sweepO_wide_T(const double* in, double* out, int pitch, const Phys& p, const SweepCfg& cfg, const Bc2& bc,
                         const FinLines& fin, const SweepPlan& plan, hipStream_t st, const FrameSync& fs, const unsigned* lease) {
    static_assert(wide_strips_compiled(0, T) && wide_strips_compiled(1, T), "see wide_strips_compiled");
    switch (p.div_mode) {
        case 0: return sweepO_div<0, T, true>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
#ifndef CSIM_ISA_PROBE
        case 1: return sweepO_div<1, T, true>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
#endif
        default: return hipErrorInvalidValue;
    }
}

}  // namespace csim
