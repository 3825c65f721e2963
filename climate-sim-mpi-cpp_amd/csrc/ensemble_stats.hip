// ensemble_stats.hip — per-cell statistics over the members of an ensemble (csim_ensemble_stats*, host side in
// ensemble_diag.cpp).  Needs only the slab layout of ensemble.hpp, not the sweep core (sweep_core.hpp).
//
// For every cell of the reference layout (ny+2) x (nx+2), ghost ring included, with x_k member k's value:
//   s = +0; s = s + x_k (k = 0 .. B-1);  mean = s / B                  (IEEE division)
//   q = +0; d = x_k - mean; q = q + d * d (k in order);  var = q / (B - ddof)
//   min / max: fmin / fmax in member order (a NaN member is skipped unless every member is NaN)
// which is np.mean / np.var(axis=0, ddof) / np.fmin.reduce / np.fmax.reduce of the stacked members, bit for bit.
//
// A workgroup owns 64 consecutive cells, one per lane, and keeps their members in LDS as [member][lane], so that
// pass 2 re-reads them from there and the ensemble crosses HBM once.  Up to STATS_COOP_MEMBERS members the workgroup
// is one wave: pass 1 walks the members in order as they arrive, each member's 64 values one coalesced 512-B stretch
// (two where the cells wrap onto the next row), loaded a batch ahead of their use.  Above that, four waves load the
// tile into LDS together and one of them runs both passes from there.  LDS holds at most STATS_LDS_MEMBERS members
// (160 KiB, all of a CU's LDS): the members past that are read from memory in both passes.
#include "ensemble_cell.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr int STATS_BATCH = 16;      // member loads in flight per lane and batch (two batches in registers)
constexpr int STATS_COOP_BATCH = 32;  // the same for each of the four loading waves of the cooperative form
// Above this many members a one-wave workgroup's LDS (512 B per member) leaves fewer than four waves per CU, too few
// loads in flight: the cooperative form takes over, four waves loading one tile into LDS, one wave computing.
constexpr int STATS_COOP_MEMBERS = 80;

// COOP = false: one wave, pass 1 as the members arrive.  COOP = true: 256 threads; the four waves load members
// [0, kl) into LDS, then wave 0 alone runs both passes from there (members from kl on come from memory).
template <bool COOP>
__global__ __launch_bounds__(COOP ? 256 : 64) void k_ensemble_stats(const double* __restrict__ f, int nx2, int ncells,
                                                                    int pitch, long slab, int members, int kl,
                                                                    double den, double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double held[];  // [kl][64]
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 64 + lane;
    const bool valid = c < ncells;
    const DenseCell dc = dense_cell(c, nx2, ncells);
    const double* __restrict__ p = cell_ptr(f, dc.i, dc.j, pitch);

    double s = 0.0, lo = __builtin_nan(""), hi = __builtin_nan("");  // fmin(NaN, x) = x
    if (COOP) {
        // members wave, wave + 4, ...: each load instruction of the four waves is one member's 512-B stretch
        const int wave = threadIdx.x >> 6;
        for (int kb = wave; kb < kl; kb += 4 * STATS_COOP_BATCH) {
            double x[STATS_COOP_BATCH];
#pragma unroll
            for (int u = 0; u < STATS_COOP_BATCH; ++u)
                x[u] = p[static_cast<ptrdiff_t>(min(kb + 4 * u, kl - 1)) * slab];
#pragma unroll
            for (int u = 0; u < STATS_COOP_BATCH; ++u)
                if (kb + 4 * u < kl) held[(kb + 4 * u) * 64 + lane] = x[u];
        }
        __syncthreads();
        if (wave != 0) return;
        // pass 1 in member order: LDS, then (past kl) memory
#pragma unroll 8
        for (int k = 0; k < kl; ++k) {
            const double x = held[k * 64 + lane];
            s = s + x;
            lo = fmin(lo, x);
            hi = fmax(hi, x);
        }
        for (int k = kl; k < members; ++k) {
            const double x = p[static_cast<ptrdiff_t>(k) * slab];
            s = s + x;
            lo = fmin(lo, x);
            hi = fmax(hi, x);
        }
    } else {
        // pass 1: sum, min, max in member order as the members arrive, a batch ahead; members [0, kl) kept in LDS
        double x[STATS_BATCH], y[STATS_BATCH];
#pragma unroll
        for (int u = 0; u < STATS_BATCH; ++u) x[u] = p[static_cast<ptrdiff_t>(min(u, members - 1)) * slab];
        for (int kb = 0; kb < members; kb += STATS_BATCH) {
            const int nb = kb + STATS_BATCH;
            if (nb < members) {
#pragma unroll
                for (int u = 0; u < STATS_BATCH; ++u)
                    y[u] = p[static_cast<ptrdiff_t>(min(nb + u, members - 1)) * slab];
            }
#pragma unroll
            for (int u = 0; u < STATS_BATCH; ++u) {
                const int k = kb + u;
                if (k < members) {  // wave-uniform
                    s = s + x[u];
                    lo = fmin(lo, x[u]);
                    hi = fmax(hi, x[u]);
                    if (k < kl) held[k * 64 + lane] = x[u];
                }
            }
#pragma unroll
            for (int u = 0; u < STATS_BATCH; ++u) x[u] = y[u];
        }
    }
    const double mean = s / static_cast<double>(members);

    // pass 2: squared deviations in member order, from LDS (each lane reads only its own column: no barrier in the
    // one-wave form, the barrier above in the cooperative one)
    double q = 0.0;
#pragma unroll 8
    for (int k = 0; k < kl; ++k) {
        const double d = held[k * 64 + lane] - mean;
        q = q + d * d;
    }
    for (int k = kl; k < members; ++k) {
        const double d = p[static_cast<ptrdiff_t>(k) * slab] - mean;
        q = q + d * d;
    }
    if (valid) {
        out[c] = mean;
        out[static_cast<size_t>(ncells) + c] = q / den;
        out[2 * static_cast<size_t>(ncells) + c] = lo;
        out[3 * static_cast<size_t>(ncells) + c] = hi;
    }
}

template <bool COOP>
hipError_t launch_stats(const EnsGeom& g, const double* f, int ddof, double* out, hipStream_t st) {
    const int nx2 = g.nx + 2;
    const int ncells = nx2 * (g.ny + 2);
    const int kl = g.members < STATS_LDS_MEMBERS ? g.members : STATS_LDS_MEMBERS;
    const size_t lds = sizeof(double) * 64 * static_cast<size_t>(kl);
    const hipError_t attr = dynamic_lds_once<k_ensemble_stats<COOP>>(sizeof(double) * 64 * STATS_LDS_MEMBERS);
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(k_ensemble_stats<COOP>, dim3((ncells + 63) / 64), dim3(COOP ? 256 : 64), lds, st, f, nx2,
                       ncells, g.pitch, g.slab, g.members, kl, static_cast<double>(g.members - ddof), out);
    return hipGetLastError();
}

}  // namespace

hipError_t ens_launch_stats(const EnsGeom& g, const double* f, int ddof, double* out, hipStream_t st) {
    return g.members > STATS_COOP_MEMBERS ? launch_stats<true>(g, f, ddof, out, st)
                                          : launch_stats<false>(g, f, ddof, out, st);
}

}  // namespace csim
