// ensemble.hip — gfx950 kernels of the batched stepper (csim_ensemble_*; host side: ensemble.cpp and the units behind
// ensemble_host.hpp).
//
// Many small members fill the GPU together: every launch below covers all members (the multi-step sweep: all
// members of one upwind-sign class), so a pass costs the same few launches whatever B is.  The multi-step sweep
// shares the single stepper's march (sweepO_march and its edge bodies: sweep_core.hpp, the only part of the sweep
// this file includes) and adds the member indexing around it.  Every member is a single-rank field with four
// physical sides: the edge bodies do the boundary work inside the pass, nothing is exchanged.
#include "sweep_core.hpp"

#include "ensemble.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

// Per-member argument block.  Laid out as a launch's SweepArgs so that the march's LateArgs, pointed at the member's
// entry instead of the kernel-argument segment, reads that member's FinLines from it; the kernels read the member's
// Phys from it too.  Only `p` and `fin` are used.
typedef SweepArgs EnsEntry;
typedef const EnsEntry __attribute__((address_space(4))) * EntryPtr;

__device__ __forceinline__ EntryPtr entry(const void* table, int m) {
    return (EntryPtr)(reinterpret_cast<const EnsEntry*>(table) + m);  // scalar loads: m is wave-uniform
}

__device__ __forceinline__ Phys member_phys(EntryPtr e) {
#if defined(__HIP_DEVICE_COMPILE__)
    return e->p;
#else
    (void)e;  // the host pass of the compiler has no constant address space to copy from
    return Phys{};
#endif
}

struct EnsArgs {
    int nx, ny, pitch, nstrips, nchunks, ry, count;
    long slab;
    const int* members;  // the launch's members (one sign class)
    const void* table;
    Bc2 bc;
    int fin;
};

// T steps per pass over every (member, strip, chunk) tile of the launch.  The tile's body is chosen exactly as in
// k_sweepO_dpp (whole-field launch, all four sides physical).
template <int DIV, int T, int SX, int SY>
__global__ __launch_bounds__(256) void k_ensemble_sweepO(const double* __restrict__ in, double* __restrict__ out,
                                                         EnsArgs a) {
    constexpr int TP = OverlapGeom<T>::TP;
    constexpr int STRIDE = OverlapGeom<T>::STRIDE;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int per = a.nstrips * a.nchunks;
    const int tile = blockIdx.x * 4 + wave;
    const int slot = tile / per;
    if (slot >= a.count) return;  // wave-uniform
    typedef const int __attribute__((address_space(4))) * IntPtr;
    const int m = __builtin_amdgcn_readfirstlane(((IntPtr)a.members)[slot]);
    const EntryPtr e = entry(a.table, m);
    const Phys p = member_phys(e);
    LateArgs late;
    late.a = e;
    const ptrdiff_t off = static_cast<ptrdiff_t>(m) * a.slab;
    const double* __restrict__ min_ = in + off;
    double* __restrict__ mout = out + off;
    const int nx = a.nx, ny = a.ny, pitch = a.pitch, nstrips = a.nstrips;
    const int local = tile - slot * per;
    const int strip = local % nstrips;
    const int chunk = local / nstrips;
    const bool first = strip == 0, last = strip == nstrips - 1;
    const int jb = 1 + chunk * a.ry;
    const int je = min(jb + a.ry - 1, ny);
    const int g0 = strip * STRIDE - TP;
    const int kl = first ? a.bc.kind[CSIM_LEFT] : 3;
    const int kr = g0 + WAVE_COLS > nx ? a.bc.kind[CSIM_RIGHT] : 3;
    const int kb = a.bc.kind[CSIM_BOTTOM], kt = a.bc.kind[CSIM_TOP];
    const bool fin_frame = a.fin && (first || last || jb == 1 || je == ny);
    const bool rows = jb - (T - 1) < 1 || je + (T - 1) > ny;
    const bool edge = kl != 3 || kr != 3 || rows || fin_frame;
#define CSIM_MARCH(MODE_) \
    sweepO_march<DIV, T, MODE_, SX, SY>(min_, mout, nx, ny, pitch, jb, je, g0, lane, kl, kr, p, kb, kt, late, fin_frame, first, last, false)
    if (edge) {
        __builtin_amdgcn_s_setprio(3);
        int col_case = 0;
        if (kl != 3 && kr != 3)
            col_case = 7;
        else if (kl != 3)
            col_case = kl == CSIM_BC_NEUMANN ? 2 : 1;
        else if (kr != 3)
            col_case = (kr == CSIM_BC_NEUMANN ? 5 : 3) + (nx & 1);
        if (!SPECIALISE_EDGES<DIV, T>::value || rows || col_case == 7) col_case = -1;
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
        if (p.fast_thr > 0.0) redo = CSIM_MARCH(M_FAST);
        if (redo) {
            keep_branch();
            CSIM_MARCH(M_PLAIN);
        }
    }
#undef CSIM_MARCH
}

// One reference step of every member (remainder steps of a run, and members smaller than the pass depth): one
// thread per interior cell, blockIdx.y = member.  The ghost ring is the ghost fill's (both buffers), as in the
// single stepper's one-step passes.
template <int DIV>
__global__ __launch_bounds__(256) void k_ensemble_step(const double* __restrict__ in, double* __restrict__ out,
                                                       int nx, int ny, int pitch, long slab, const void* table) {
    const int m = blockIdx.y;
    const long t = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= static_cast<long>(nx) * ny) return;
    const int i = static_cast<int>(t % nx) + 1, j = static_cast<int>(t / nx) + 1;
    const EntryPtr e = entry(table, m);
    const Phys p = member_phys(e);
    const ptrdiff_t o = static_cast<ptrdiff_t>(m) * slab + at(i, j, pitch);
    const double c = in[o];
    out[o] = cell<DIV>(c, in[o - 1], in[o + 1], in[o - pitch], in[o + pitch], p);
}

// apply_boundary (reference src/boundary.cpp:12-54) of every member, four physical sides, written to a and b: the
// single stepper's ghost-fill rule (ghost_fill_cell) per member, blockIdx.y = member.  fin: the Neumann ghosts take the
// member's FinLines (the adjacent interior line of the state before the last step) instead of the field's own line.
__global__ __launch_bounds__(256) void k_ensemble_ghost(double* __restrict__ a, double* __restrict__ b, int nx, int ny,
                                                        int pitch, long slab, Bc2 bc, const void* table, int fin) {
    const int m = blockIdx.y;
    GhostDev g;
    for (int s = 0; s < 4; ++s) {
        g.bc[s] = bc.kind[s];
        g.phys[s] = 1;
        g.recv[s] = nullptr;
        g.adj[s] = nullptr;
    }
    g.value = bc.value;
    g.ext_depth = 0;
    if (fin) {
        const EntryPtr e = entry(table, m);
        for (int s = 0; s < 4; ++s) g.adj[s] = e->fin.line[s];
    }
    const ptrdiff_t off = static_cast<ptrdiff_t>(m) * slab;
    ghost_fill_cell(a + off, b + off, nx, ny, pitch, g, blockIdx.x * 256 + threadIdx.x);
}

inline int cdivl(long a, long b) { return static_cast<int>((a + b - 1) / b); }

template <int DIV, int T>
hipError_t ens_sweepO_div(const EnsGeom& g, const double* in, double* out, const void* table, const int* members,
                          int count, int cls, bool fin, hipStream_t st) {
    constexpr int STRIDE = OverlapGeom<T>::STRIDE;
    EnsArgs a;
    a.nx = g.nx, a.ny = g.ny, a.pitch = g.pitch, a.count = count, a.slab = g.slab;
    a.nstrips = cdivl(g.nx, STRIDE);
    a.ry = ens_chunk_rows(T, count, a.nstrips, g.ny);  // sweep_plan.cpp
    a.nchunks = cdivl(g.ny, a.ry);
    a.members = members, a.table = table;
    for (int s = 0; s < 4; ++s) a.bc.kind[s] = g.bc[s];
    a.bc.value = g.value;
    a.fin = fin ? 1 : 0;
    const long tiles = static_cast<long>(count) * a.nstrips * a.nchunks;
    if (tiles == 0) return hipSuccess;
    const dim3 grid(cdivl(tiles, 4)), block(256);
#define CSIM_LAUNCH_E(SXV, SYV) hipLaunchKernelGGL((k_ensemble_sweepO<DIV, T, SXV, SYV>), grid, block, 0, st, in, out, a)
    switch (cls) {
        case 8: if constexpr (DIV <= 1) CSIM_LAUNCH_E(2, 2); break;
        case 7: if constexpr (DIV <= 1) CSIM_LAUNCH_E(2, 1); break;
        case 6: if constexpr (DIV <= 1) CSIM_LAUNCH_E(2, 0); break;
        case 5: if constexpr (DIV <= 1) CSIM_LAUNCH_E(1, 2); break;
        case 2: if constexpr (DIV <= 1) CSIM_LAUNCH_E(0, 2); break;
        case 4: CSIM_LAUNCH_E(1, 1); break;
        case 3: CSIM_LAUNCH_E(1, 0); break;
        case 1: CSIM_LAUNCH_E(0, 1); break;
        default: CSIM_LAUNCH_E(0, 0); break;
    }
#undef CSIM_LAUNCH_E
    return hipGetLastError();
}

}  // namespace

size_t ens_entry_bytes() { return sizeof(EnsEntry); }

void ens_entry_fill(void* host_entry, const Phys& p, double* const fin_lines[4]) {
    EnsEntry e{};
    e.p = p;
    for (int s = 0; s < 4; ++s) e.fin.line[s] = fin_lines[s];
    *reinterpret_cast<EnsEntry*>(host_entry) = e;
}

hipError_t ens_launch_sweepO(const EnsGeom& g, const double* in, double* out, const void* table, const int* members,
                             int count, int cls, bool fin, hipStream_t st) {
    switch (g.div_mode) {
        case 0: return ens_sweepO_div<0, ENS_DEPTH>(g, in, out, table, members, count, cls, fin, st);
        case 1: return ens_sweepO_div<1, ENS_DEPTH>(g, in, out, table, members, count, cls, fin, st);
        default: return ens_sweepO_div<2, ENS_DEPTH>(g, in, out, table, members, count, cls, fin, st);
    }
}

hipError_t ens_launch_step(const EnsGeom& g, const double* in, double* out, const void* table, hipStream_t st) {
    const dim3 grid(cdivl(static_cast<long>(g.nx) * g.ny, 256), g.members), block(256);
    switch (g.div_mode) {
        case 0: hipLaunchKernelGGL(k_ensemble_step<0>, grid, block, 0, st, in, out, g.nx, g.ny, g.pitch, g.slab, table); break;
        case 1: hipLaunchKernelGGL(k_ensemble_step<1>, grid, block, 0, st, in, out, g.nx, g.ny, g.pitch, g.slab, table); break;
        default: hipLaunchKernelGGL(k_ensemble_step<2>, grid, block, 0, st, in, out, g.nx, g.ny, g.pitch, g.slab, table); break;
    }
    return hipGetLastError();
}

hipError_t ens_launch_ghost_fill(const EnsGeom& g, double* a, double* b, const void* table, bool fin, hipStream_t st) {
    Bc2 bc;
    for (int s = 0; s < 4; ++s) bc.kind[s] = g.bc[s];
    bc.value = g.value;
    const dim3 grid(cdivl(std::max(g.nx, g.ny) + 1, 256), g.members), block(256);
    hipLaunchKernelGGL(k_ensemble_ghost, grid, block, 0, st, a, b, g.nx, g.ny, g.pitch, g.slab, bc, table, fin ? 1 : 0);
    return hipGetLastError();
}

}  // namespace csim
