// obs_wave.hpp — the wave that owns an observation: what the serial analysis (ensemble_assim.hip), the local analysis and
// the LETKF (ensemble_local.hip, ensemble_letkf.hip) and the forecast impact (ensemble_impact.hip) promise to agree on,
// said once.  Two halves:
//   h_k       the M forecast members seen by the observation at plan position q, in LDS: its cell (a point observation)
//             or linear_h (a linear one, csim_obs_network_create_linear) — obs_h<LIN>; their mean, obs_hbar; and
//             for_obs_form, which chooses the instantiation and its LDS on the host.
//   windows   an observation's window clipped to the interior, its cells row-major, and the localisation of a cell
//             (obs_window, window_cell, window_rho): the update and the impact walk the same cells of the same window,
//             and the list builders look rho up the same way.
// Needs the cell addressing of ensemble_cell.hpp; the device pieces are force-inlined into their kernels.
#pragma once

#include "ensemble_cell.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

// LDS of a wave that runs linear_h: M values of h, the tile of 64 members x (tmax | 1) values, 64 tap offsets
inline size_t linear_lds(const AssimArgs& a) {
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

// One wave: h_k of the M forecast members for the observation at plan position q into sh[0 .. M).  LIN: linear_h, its
// tile behind the M values (linear_lds); else the observation's cell of every member.  Ends with a barrier.
template <bool LIN>
__device__ __forceinline__ void obs_h(const double* __restrict__ f, int pitch, long slab, const AssimArgs& a, int q,
                                      double* __restrict__ sh) {
    const int M = a.forecast, t = a.truth_member;
    const double* p = cell_ptr(f, a.obs.i[q], a.obs.j[q], pitch);
    if constexpr (LIN) {
        linear_h(p, slab, a, q, sh, sh + M);
    } else {
        for (int k = threadIdx.x; k < M; k += 64) sh[k] = p[static_cast<ptrdiff_t>(forecast_member(k, t)) * slab];
        __syncthreads();
    }
}

// the mean of obs_h's values, every lane the same: a running sum from +0 in member order
__device__ __forceinline__ double obs_hbar(const double* sh, int M) {
    double s = 0.0;
    for (int k = 0; k < M; ++k) s = s + sh[k];
    return s / static_cast<double>(M);
}

// launch(lin, lds) with std::true_type and linear_lds for a linear network, std::false_type and point_lds for points:
// the host's choice of the instantiation of a kernel that calls obs_h<LIN>
template <class F>
hipError_t for_obs_form(const AssimArgs& a, size_t point_lds, F&& launch) {
    if (a.tstart) {
        if (a.tmax < 1 || a.tmax > OBS_MAX_TAPS) return hipErrorInvalidValue;
        return launch(std::true_type{}, linear_lds(a));
    }
    return launch(std::false_type{}, point_lds);
}

// rho of the cell (di, dj) away from its observation, |di| <= lx and |dj| <= ly: the host's Gaspari-Cohn table
__device__ __forceinline__ double window_rho(const double* __restrict__ rho, int lx, int ly, int di, int dj) {
    return rho[static_cast<size_t>(dj + ly) * (2 * lx + 1) + (di + lx)];
}

// The window of the observation at (io, jo), clipped to the interior: rows of W cells from (i0, j0), `cells` in all,
// numbered row-major.  I: int where the caller bounds a window to 2^31 cells, else long
template <class I>
struct ObsWindow {
    int io, jo, i0, j0;
    I W, cells;
};
template <class I>
__device__ __forceinline__ ObsWindow<I> obs_window(int io, int jo, int lx, int ly, int nx, int ny) {
    const int i0 = max(1, io - lx), i1 = min(nx, io + lx), j0 = max(1, jo - ly), j1 = min(ny, jo + ly);
    const I W = i1 - i0 + 1;
    return {io, jo, i0, j0, W, W * (j1 - j0 + 1)};
}

// cell e of a window and its rho; e past the end is the last cell again (the caller stores, or adds, nothing there)
struct WindowCell {
    int ci, cj;
    double rho;
};
template <class I>
__device__ __forceinline__ WindowCell window_cell(const ObsWindow<I>& win, I e, const double* __restrict__ rho, int lx,
                                                  int ly) {
    e = e < win.cells - 1 ? e : win.cells - 1;
    const int row = static_cast<int>(e / win.W);
    const int ci = win.i0 + static_cast<int>(e - row * win.W), cj = win.j0 + row;
    return {ci, cj, window_rho(rho, lx, ly, ci - win.io, cj - win.jo)};
}

}  // namespace

}  // namespace csim
