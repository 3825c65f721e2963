// ensemble_assim.hip — the analysis of csim_ensemble_assimilate (host side in ensemble_da.cpp): the serial ensemble
// square-root filter of csim.h, localised with the host's Gaspari-Cohn table.  Needs only the slab layout of
// ensemble.hpp.
//
// The host sorts the observations into levels (csim_ensemble_assim_plan); observations of one level have disjoint
// windows and none lies in another's window, so each level is one batch of independent rank-1 updates, two launches:
//   assim_prior   one wave per observation: h_k of the M forecast members, hbar, h'_k (to `hp`), p, d, alpha, delta.
//                 It runs apart from the update so that no workgroup of an observation can overwrite the observed cell
//                 while another workgroup of that observation still reads it.  Linear observations (a.tstart, the
//                 taps of csim_obs_network_create_linear) differ only in h_k = sum_s w_s x_k(anchor + tap s):
//                 obs_h of obs_wave.hpp; the taps lie outside every other window of the level, so the same holds for
//                 them.
//   assim_update  one wave per 64 cells of one observation's window (blockIdx.y: the observation, blockIdx.x: which
//                 64 cells of its window clipped to the interior, row-major), so h'_k and the scalars are the same in
//                 every lane of a wave, and lanes that follow i within a window row load each member coalesced.
//                 M <= 64: each lane reads its cell of every member once into registers and writes it once.  M > 64:
//                 three passes over the members (mean, covariance, update); a window's members stay in L2 between them.
// Screening (a.status, csim_ensemble_assimilate_screened): a byte per plan position; the block of an observation whose
// byte is not 0 leaves at once in assim_prior and skips it in assim_update, so it reads and writes nothing.  The
// pointer is a kernel argument (null: as before), the test a scalar one: no instantiation of its own is needed.
// Forecast members, cell addressing, the register and memory forms of a cell's members and their running sums, the
// covariance with h'_k among them, are those of ensemble_cell.hpp; a window's cells and their rho are those of
// obs_wave.hpp, which the impact walks too; the update is summed and rounded the same way, / and sqrt
// are IEEE fp64 (no fast-math), so the numpy restatement of the csim.h block gives the same bits.  Only interior cells
// of the forecast members are written; ghost rings, member t and the other ping-pong buffer are never touched.
#include <algorithm>

#include "obs_wave.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr int ASSIM_GRID_Y = 65535;  // observations per launch row (larger batches loop)

// LIN: linear observations (obs_h); the point instantiation is the kernel as it was before they existed
template <bool LIN>
__global__ __launch_bounds__(64) void k_assim_prior(const double* __restrict__ f, int pitch, long slab, AssimArgs a,
                                                    int first) {
    extern __shared__ double sh[];  // M values (dynamic: a small ensemble does not pay for 1024); LIN: linear_lds
    const int lane = threadIdx.x;
    const int M = a.forecast;
    const int q = first + blockIdx.x;
    if (a.status && a.status[q]) return;  // screened out: the whole block, before any barrier
    obs_h<LIN>(f, pitch, slab, a, q, sh);
    const double hbar = obs_hbar(sh, M);
    __syncthreads();
    double* __restrict__ hp = a.hp + static_cast<size_t>(blockIdx.x) * M;
    for (int k = lane; k < M; k += 64) {
        const double v = sh[k] - hbar;
        sh[k] = v;
        hp[k] = v;
    }
    __syncthreads();
    double ss = 0.0;
    for (int k = 0; k < M; ++k) ss = ss + sh[k] * sh[k];
    const double pv = ss / static_cast<double>(M - 1);
    const double r = a.obs.r[q];
    const double d = pv + r;
    if (lane == 0) {
        a.scal[3 * static_cast<size_t>(q)] = d;
        a.scal[3 * static_cast<size_t>(q) + 1] = 1.0 / (1.0 + sqrt(r / d));
        a.scal[3 * static_cast<size_t>(q) + 2] = a.obs.y[q] - hbar;
        if (a.prior) {
            const size_t o = 2 * static_cast<size_t>(a.obs.idx[q]);
            a.prior[o] = hbar;
            a.prior[o + 1] = pv;
        }
    }
}

// P > 0: the members in registers (P >= M); P = 0: re-read.  h'_k is staged in LDS (M values, dynamic) and read again
// after a barrier for the update, so that the compiler does not keep all M of them live next to the members.  With
// h'_k held in registers instead, P = 64 took 256 VGPRs plus AGPRs (one wave per SIMD); this form compiles to 177
// VGPRs and no AGPRs (two waves per SIMD), DESIGN §7f.  P from for_step
template <int P>
__global__ __launch_bounds__(64) void k_assim_update(double* __restrict__ f, int nx, int ny, int pitch, long slab,
                                                     AssimArgs a, int first, int count) {
    extern __shared__ double sh[];  // M values
    const int lane = threadIdx.x;
    const int M = a.forecast, t = a.truth_member;
    const double cden = static_cast<double>(M - 1);
    for (int o = blockIdx.y; o < count; o += gridDim.y) {
        const int q = first + o;
        if (a.status && a.status[q]) continue;  // screened out: the same in every lane, nothing of it is read
        const ObsWindow<long> win = obs_window<long>(a.obs.i[q], a.obs.j[q], a.lx, a.ly, nx, ny);
        const long cells = win.cells;
        if (static_cast<long>(blockIdx.x) * 64 >= cells) continue;  // the same in every lane
        const double d = a.scal[3 * static_cast<size_t>(q)], alpha = a.scal[3 * static_cast<size_t>(q) + 1];
        const double delta = a.scal[3 * static_cast<size_t>(q) + 2];
        __syncthreads();  // the last observation's readers of sh are done
        for (int k = lane; k < M; k += 64) sh[k] = a.hp[static_cast<size_t>(o) * M + k];
        __syncthreads();
        for (long e0 = static_cast<long>(blockIdx.x) * 64; e0 < cells; e0 += static_cast<long>(gridDim.x) * 64) {
            const auto [ci, cj, rho] = window_cell(win, e0 + lane, a.rho, a.lx, a.ly);  // past the end: stores nothing
            const bool act = e0 + lane < cells && rho > 0.0;
            if constexpr (P > 0) {
                double x[P];
                const unsigned off = cell_off(ci, cj, pitch);
                load_members<P>(f, slab, off, M, t, x);
                const double c = cov_regs<P>(x, M, mean_regs<P>(x, M), sh);
                const double g = (rho * (c / cden)) / d;
                const double beta = alpha * g;
                __syncthreads();
#pragma unroll
                for (int k = 0; k < P; ++k)
                    if (act && k < M)
                        f[static_cast<size_t>(forecast_member(k, t)) * slab + off] = x[k] + (g * delta - beta * sh[k]);
            } else {
                double* p = cell_ptr(f, ci, cj, pitch);
                const double c = cov_mem<1>(p, slab, M, t, mean_mem(p, slab, 0u, M, t), sh);
                const double g = (rho * (c / cden)) / d;
                const double beta = alpha * g;
                if (act)
                    for (int k = 0; k < M; ++k) {
                        double* pk = p + static_cast<ptrdiff_t>(forecast_member(k, t)) * slab;
                        *pk = *pk + (g * delta - beta * sh[k]);
                    }
            }
        }
    }
}

// one thread per interior cell (lanes along i), two passes over the members
__global__ __launch_bounds__(256) void k_assim_inflate(double* __restrict__ f, int nx, int ny, int pitch, long slab,
                                                       int M, int t, double lm1) {
    const long cells = static_cast<long>(nx) * ny;
    for (long e = static_cast<long>(blockIdx.x) * 256 + threadIdx.x; e < cells;
         e += static_cast<long>(gridDim.x) * 256) {
        const Cell c = cell_of(e, nx, pitch);
        double* p = cell_ptr(f, c.i, c.j, pitch);
        const double xbar = mean_mem(p, slab, 0u, M, t);
        for (int k = 0; k < M; ++k) {
            double* pk = p + static_cast<ptrdiff_t>(forecast_member(k, t)) * slab;
            const double x = *pk;
            *pk = x + lm1 * (x - xbar);
        }
    }
}

// one thread per observation
__global__ __launch_bounds__(256) void k_assim_post(const double* __restrict__ f, int pitch, long slab, AssimArgs a,
                                                    int nobs, double* __restrict__ post) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nobs) return;
    const int M = a.forecast, t = a.truth_member;
    const double* p = cell_ptr(f, a.obs.i[q], a.obs.j[q], pitch);
    const double m = mean_mem(p, slab, 0u, M, t);
    const size_t o = 2 * static_cast<size_t>(a.obs.idx[q]);
    post[o] = m;
    post[o + 1] = var_mem(p, slab, 0u, M, t, m);
}

// the same for linear observations, one wave per observation: mv of csim_ensemble_relax applied to h_k
__global__ __launch_bounds__(64) void k_assim_post_linear(const double* __restrict__ f, int pitch, long slab,
                                                          AssimArgs a, double* __restrict__ post) {
    extern __shared__ double sh[];  // linear_lds
    const int M = a.forecast;
    const int q = blockIdx.x;
    obs_h<true>(f, pitch, slab, a, q, sh);
    double m, v;
    mv(sh, M, m, v);
    if (threadIdx.x == 0) {
        const size_t o = 2 * static_cast<size_t>(a.obs.idx[q]);
        post[o] = m;
        post[o + 1] = v;
    }
}

}  // namespace

hipError_t ens_launch_assim_prior(const EnsGeom& g, const double* f, const AssimArgs& a, int first, int count,
                                  hipStream_t st) {
    if (count <= 0) return hipSuccess;
    if (a.forecast < 2 || a.forecast > ASSIM_MAX_MEMBERS) return hipErrorInvalidValue;
    return for_obs_form(a, sizeof(double) * a.forecast, [&](auto lin, size_t lds) {
        hipLaunchKernelGGL(k_assim_prior<decltype(lin)::value>, dim3(count), dim3(64), lds, st, f, g.pitch, g.slab, a,
                           first);
        return hipGetLastError();
    });
}

hipError_t ens_launch_assim_update(const EnsGeom& g, double* f, const AssimArgs& a, int first, int count,
                                   long wcells, hipStream_t st) {
    if (count <= 0 || wcells <= 0) return hipSuccess;
    const int M = a.forecast;
    if (M < 2 || M > ASSIM_MAX_MEMBERS || wcells > 64L * 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((wcells + 63) / 64), static_cast<unsigned>(std::min(count, ASSIM_GRID_Y)));
    return for_step(M, [&](auto s) {
        hipLaunchKernelGGL(k_assim_update<decltype(s)::value>, grid, dim3(64), sizeof(double) * M, st, f, g.nx, g.ny,
                           g.pitch, g.slab, a, first, count);
        return hipGetLastError();
    });
}

hipError_t ens_launch_assim_inflate(const EnsGeom& g, double* f, int forecast, int truth_member, double lm1,
                                    hipStream_t st) {
    const long cells = static_cast<long>(g.nx) * g.ny;
    const unsigned blocks = static_cast<unsigned>(std::min<long>((cells + 255) / 256, 65536L));
    hipLaunchKernelGGL(k_assim_inflate, dim3(blocks), dim3(256), 0, st, f, g.nx, g.ny, g.pitch, g.slab, forecast,
                       truth_member, lm1);
    return hipGetLastError();
}

hipError_t ens_launch_assim_post(const EnsGeom& g, const double* f, const AssimArgs& a, int nobs, double* post,
                                 hipStream_t st) {
    if (nobs <= 0) return hipSuccess;
    if (a.tstart) {
        if (a.tmax < 1 || a.tmax > OBS_MAX_TAPS) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_assim_post_linear, dim3(nobs), dim3(64), linear_lds(a), st, f, g.pitch, g.slab, a, post);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_assim_post, dim3((nobs + 255) / 256), dim3(256), 0, st, f, g.pitch, g.slab, a, nobs, post);
    return hipGetLastError();
}

}  // namespace csim
