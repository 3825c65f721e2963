// ensemble_linear.hpp — the operator of a linear observation (csim_obs_network_create_linear) for one wave: what the
// analysis (ensemble_assim.hip) and the impact capture (ensemble_impact.hip) share, said once.  Needs the cell addressing
// of ensemble_cell.hpp; force-inlined into its kernels.
#pragma once

#include "ensemble_cell.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

// LDS of a wave that runs linear_h: M values of h, the tile of 64 members x (tmax | 1) values, 64 tap offsets
size_t linear_lds(const AssimArgs& a) {
    return sizeof(double) * a.forecast + sizeof(double) * 64 * (a.tmax | 1) + sizeof(int) * 64;
}

// One wave: h_k = sum_s w_s x_k(anchor + tap s) of the M forecast members for the observation at plan position q, into
// sh[0 .. M); p: the anchor's cell in member 0; tile: 64 (tmax | 1) doubles and 64 ints behind sh.  64 members at a
// time: the 64 x nt values go to the tile with the lanes along the taps (element e = m nt + s in lane e % 64), so the
// lanes of a load read runs of neighbouring cells of a few members: a footprint's row is one or two cache lines per
// member, where one lane per member would make every load 64 lines `slab` apart.  Then lane m folds row m of the tile
// in tap order, a running sum from +0, every product rounded.  Rows are ld = nt | 1 doubles apart: odd, so the 32
// lanes of a ds_read_b64 group hit 32 different bank pairs.  Ends with a barrier.
__device__ __forceinline__ void linear_h(const double* __restrict__ p, long slab, const AssimArgs& a, int q,
                                         double* __restrict__ sh, double* __restrict__ tile) {
    const int lane = threadIdx.x;
    const int M = a.forecast, t = a.truth_member;
    const int s0 = a.tstart[q], nt = a.tstart[q + 1] - s0, ld = nt | 1;
    const double* __restrict__ w = a.tw + s0;
    int* offs = reinterpret_cast<int*>(tile + 64 * (a.tmax | 1));
    if (lane < nt) offs[lane] = a.toff[s0 + lane];
    __syncthreads();
    const int dm = 64 / nt, ds = 64 - dm * nt;  // what 64 elements further means for (m, s)
    for (int k0 = 0; k0 < M; k0 += 64) {
        const int nm = min(64, M - k0), n = nm * nt;
        int m = lane / nt, s = lane - m * nt;
        for (int e = lane; e < n; e += 64) {
            const int k = k0 + m;
            tile[m * ld + s] = p[static_cast<ptrdiff_t>(forecast_member(k, t)) * slab + offs[s]];
            m += dm, s += ds;
            if (s >= nt) s -= nt, ++m;
        }
        __syncthreads();
        if (lane < nm) {
            double h = 0.0;
            for (int u = 0; u < nt; ++u) h = h + w[u] * tile[lane * ld + u];
            sh[k0 + lane] = h;
        }
        __syncthreads();  // sh is complete, and the tile is free for the next 64 members
    }
}

}  // namespace

}  // namespace csim
