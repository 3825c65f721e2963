// ensemble_impact.hip — the kernels of the per-observation forecast impact (csim_obs_network_impact_capture and
// csim_ensemble_obs_impact in include/csim.h, host side in ensemble_obs_impact.cpp): ensemble forecast sensitivity to
// observations.  Needs only the slab layout of ensemble.hpp.  Both kernels only read the members.
//
//   k_impact_capture  one wave per observation (plan position q), as k_assim_prior: h_k of the M forecast members into
//                 LDS and their mean ha exactly as there (obs_h and obs_hbar of obs_wave.hpp),
//                 and a_k = h_k - ha to the network's storage, M doubles per plan position, written coalesced.  Lane 0
//                 snapshots dn = (y - hb) / r and the status byte.  The block of an observation that was not used
//                 stores its byte and leaves before any barrier: nothing else of it is ever read.
//   k_obs_impact  one wave per observation, grid-stride over the plan positions.  a_k is staged in LDS (M doubles,
//                 dynamic) as k_assim_update stages h'_k; the lanes go along the window's cells, row-major in the
//                 window clipped to the interior (obs_window and window_cell of obs_wave.hpp, the update's own), so
//                 each member's load coalesces along a window row.  Cell e of the
//                 window is taken by lane e % 64 in pass e / 64, and a lane adds its terms as they come: that is the
//                 lane rule of csim.h, and the xor butterfly after the last pass is its combination.  Lanes past the
//                 window's end redo the last cell and add +0; a cell with rho == 0 adds +0 whatever it holds.  (A
//                 running sum that started from +0 is never -0, so adding +0 leaves its bits.)  An observation that
//                 was not used is skipped by the whole block before any barrier, and gets +0.
//                 P > 0: the members in registers (load_members, mean_regs, cov_regs); P = 0: re-read (mean_mem,
//                 cov_mem), as in k_assim_update.  Nothing is written back, so the members are dead after the
//                 covariance: P = 64 needs fewer registers than the update.
// One wave owns one observation from its first load to its store, so neither the grid nor the batch shows in a result.
// Every product is rounded, no FMA contraction, / IEEE fp64.
#include <algorithm>

#include "obs_wave.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr int IMPACT_GRID = 4096;  // waves of k_obs_impact, at most: 16 per CU, each loops over its observations

template <bool LIN>
__global__ __launch_bounds__(64) void k_impact_capture(const double* __restrict__ f, int pitch, long slab, AssimArgs a,
                                                       ImpactCapture c) {
    extern __shared__ double sh[];  // M values; LIN: linear_lds
    const int lane = threadIdx.x;
    const int M = a.forecast;
    const int q = blockIdx.x;
    const unsigned char st = c.status ? c.status[q] : 0;
    if (lane == 0) c.snap[q] = st;
    if (st) return;  // not used: the whole block, before any barrier
    obs_h<LIN>(f, pitch, slab, a, q, sh);
    const double ha = obs_hbar(sh, M);
    double* __restrict__ pert = c.pert + static_cast<size_t>(q) * M;
    for (int k = lane; k < M; k += 64) pert[k] = sh[k] - ha;
    if (lane == 0) c.dn[q] = (a.obs.y[q] - c.bg[2 * static_cast<size_t>(a.obs.idx[q])]) / a.obs.r[q];
}

// P from for_step
template <int P>
__global__ __launch_bounds__(64) void k_obs_impact(const double* __restrict__ f, int nx, int ny, int pitch, long slab,
                                                   ImpactArgs a, double* __restrict__ out) {
    extern __shared__ double sh[];  // M values
    const int lane = threadIdx.x;
    const int M = a.forecast, t = a.truth_member, nx2 = nx + 2;
    const double cden = static_cast<double>(M - 1);
    for (int q = blockIdx.x; q < a.nobs; q += gridDim.x) {
        if (a.snap[q]) {  // not used: the same in every lane, nothing of it is read
            if (lane == 0) out[a.idx[q]] = 0.0;
            continue;
        }
        const ObsWindow<int> win = obs_window<int>(a.i[q], a.j[q], a.lx, a.ly, nx, ny);
        const int cells = win.cells;
        __syncthreads();  // the last observation's readers of sh are done
        for (int k = lane; k < M; k += 64) sh[k] = a.pert[static_cast<size_t>(q) * M + k];
        __syncthreads();
        double acc = 0.0;
        for (int e0 = 0; e0 < cells; e0 += 64) {
            const auto [ci, cj, rho] = window_cell(win, e0 + lane, a.rho, a.lx, a.ly);  // past the end: adds +0
            const bool act = e0 + lane < cells && rho > 0.0;
            double c = 0.0;
            if constexpr (P > 0) {
                double x[P];
                load_members<P>(f, slab, cell_off(ci, cj, pitch), M, t, x);
                c = cov_regs<P>(x, M, mean_regs<P>(x, M), sh);
            } else {
                const double* p = cell_ptr(f, ci, cj, pitch);
                c = cov_mem<8>(p, slab, M, t, mean_mem(p, slab, 0u, M, t), sh);
            }
            const double u = (rho * (c / cden)) * a.w[static_cast<size_t>(cj) * nx2 + ci];
            acc = acc + (act ? u : 0.0);
        }
        for (int h = 32; h >= 1; h >>= 1) acc = acc + __shfl_xor(acc, h, 64);
        if (lane == 0) out[a.idx[q]] = a.dn[q] * acc;
    }
}

}  // namespace

hipError_t ens_launch_impact_capture(const EnsGeom& g, const double* f, const AssimArgs& a, int nobs,
                                     const ImpactCapture& c, hipStream_t st) {
    if (nobs <= 0 || a.forecast < 2 || a.forecast > ASSIM_MAX_MEMBERS || !c.bg || !c.pert || !c.dn || !c.snap)
        return hipErrorInvalidValue;
    return for_obs_form(a, sizeof(double) * a.forecast, [&](auto lin, size_t lds) {
        hipLaunchKernelGGL(k_impact_capture<decltype(lin)::value>, dim3(nobs), dim3(64), lds, st, f, g.pitch, g.slab, a,
                           c);
        return hipGetLastError();
    });
}

hipError_t ens_launch_obs_impact(const EnsGeom& g, const double* f, const ImpactArgs& a, double* out, hipStream_t st) {
    const int M = a.forecast;
    if (a.nobs <= 0 || M < 2 || M > ASSIM_MAX_MEMBERS || g.slab > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(std::min(a.nobs, IMPACT_GRID)));
    return for_step(M, [&](auto s) {
        hipLaunchKernelGGL(k_obs_impact<decltype(s)::value>, grid, dim3(64), sizeof(double) * M, st, f, g.nx, g.ny,
                           g.pitch, g.slab, a, out);
        return hipGetLastError();
    });
}

}  // namespace csim
