// ensemble_relax.hip — the relaxation inflation of csim_ensemble_prior_capture / csim_ensemble_relax (host side in
// ensemble_da.cpp): relaxation to prior spread (RTPS) and to prior perturbations (RTPP), the block in csim.h.  Needs
// only the slab layout of ensemble.hpp.
//
// Every kernel: one lane per interior cell (cell_of), the forecast members of the cell in the register form or the
// memory form of ensemble_cell.hpp, chosen by for_step; the update's pass over the members is unrolled like the sums.
//   k_relax_capture  sb = sqrt(v) of mv(x), one store per cell
//   k_relax_spread   sa = sqrt(v) of mv(x), fac = sa > 0 ? alpha ((sb - sa) / sa) : +0; where fac == 0 nothing is
//                    written (outside every observation window the analysis left the bits alone, so fac is exactly +0)
//   k_relax_pert     the means of x and of the captured xb, then the update.  The register form holds x_k only: xb_k is
//                    read for its mean and read again (from L2) for the update, which keeps P = 64 at the registers of
//                    k_relax_spread instead of twice as many.
// m and v are the running sums of ensemble_cell.hpp; / and sqrt are IEEE fp64 (no fast-math), so the numpy restatement
// (tests/relax_restatement.py) gives the same bits.  Only interior cells of the forecast members are written; ghost
// rings, member t and the other ping-pong buffer are never touched.
#include <algorithm>

#include "ensemble_cell.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr long RELAX_MAX_BLOCKS = 1L << 20;  // larger fields loop

template <int P>
__global__ __launch_bounds__(64) void k_relax_capture(const double* __restrict__ f, int nx, int ny, int pitch,
                                                      long slab, int M, int t, double* __restrict__ sb) {
    const long cells = static_cast<long>(nx) * ny;
    for (long e = static_cast<long>(blockIdx.x) * 64 + threadIdx.x; e < cells; e += static_cast<long>(gridDim.x) * 64) {
        const Cell c = cell_of(e, nx, pitch);
        double v;
        if constexpr (P > 0) {
            double x[P];
            load_members<P>(f, slab, c.off, M, t, x);
            v = var_regs<P>(x, M, mean_regs<P>(x, M));
        } else {
            v = var_mem(f, slab, c.off, M, t, mean_mem(f, slab, c.off, M, t));
        }
        sb[e] = sqrt(v);
    }
}

// three waves per SIMD asked for: P = 64 then takes 168 VGPRs instead of 169, one register under the step from three
// waves to two; no other instantiation is near a step
template <int P>
__global__ __launch_bounds__(64, 3) void k_relax_spread(double* __restrict__ f, int nx, int ny, int pitch, long slab,
                                                     int M, int t, double alpha, const double* __restrict__ sb,
                                                     double* __restrict__ factor) {
    __shared__ volatile double bounce[64];
    const long cells = static_cast<long>(nx) * ny;
    for (long e = static_cast<long>(blockIdx.x) * 64 + threadIdx.x; e < cells; e += static_cast<long>(gridDim.x) * 64) {
        const Cell c = cell_of(e, nx, pitch);
        const double b = sb[e];
        if constexpr (P > 0) {
            double x[P];
            load_members<P>(f, slab, c.off, M, t, x);
            const double m = mean_regs<P>(x, M);
            const double sa = sqrt(var_regs<P>(x, M, m));
            const double fac = sa > 0.0 ? alpha * ((b - sa) / sa) : 0.0;
            if (factor) factor[static_cast<size_t>(c.j) * (nx + 2) + c.i] = fac;
            if (!(fac == 0.0)) {
                // m goes through the lane's own LDS slot and comes back with the same bits: the compiler then cannot
                // take x_k - m from the variance sum, which kept P more values live next to the members (P = 64:
                // 256 VGPRs + 38 AGPRs, one wave per SIMD)
                bounce[threadIdx.x] = m;
                const double m2 = bounce[threadIdx.x];
#pragma unroll
                for (int k = 0; k < P; ++k)
                    if (k < M) f[static_cast<size_t>(forecast_member(k, t)) * slab + c.off] = x[k] + fac * (x[k] - m2);
            }
        } else {
            const double m = mean_mem(f, slab, c.off, M, t);
            const double sa = sqrt(var_mem(f, slab, c.off, M, t, m));
            const double fac = sa > 0.0 ? alpha * ((b - sa) / sa) : 0.0;
            if (factor) factor[static_cast<size_t>(c.j) * (nx + 2) + c.i] = fac;
            if (!(fac == 0.0)) {
#pragma unroll 8
                for (int k = 0; k < M; ++k) {
                    const size_t o = static_cast<size_t>(forecast_member(k, t)) * slab + c.off;
                    const double x = f[o];
                    f[o] = x + fac * (x - m);
                }
            }
        }
    }
}

template <int P>
__global__ __launch_bounds__(64) void k_relax_pert(double* __restrict__ f, const double* __restrict__ fb, int nx,
                                                   int ny, int pitch, long slab, int M, int t, double alpha) {
    const long cells = static_cast<long>(nx) * ny;
    for (long e = static_cast<long>(blockIdx.x) * 64 + threadIdx.x; e < cells; e += static_cast<long>(gridDim.x) * 64) {
        const Cell c = cell_of(e, nx, pitch);
        const double mb = mean_mem(fb, slab, c.off, M, t);
        if constexpr (P > 0) {
            double x[P];
            load_members<P>(f, slab, c.off, M, t, x);
            const double m = mean_regs<P>(x, M);
#pragma unroll
            for (int k = 0; k < P; ++k)
                if (k < M) {
                    const size_t o = static_cast<size_t>(forecast_member(k, t)) * slab + c.off;
                    f[o] = x[k] + alpha * ((fb[o] - mb) - (x[k] - m));
                }
        } else {
            const double m = mean_mem(f, slab, c.off, M, t);
#pragma unroll 8
            for (int k = 0; k < M; ++k) {
                const size_t o = static_cast<size_t>(forecast_member(k, t)) * slab + c.off;
                const double x = f[o];
                f[o] = x + alpha * ((fb[o] - mb) - (x - m));
            }
        }
    }
}

unsigned relax_blocks(const EnsGeom& g) {
    const long cells = static_cast<long>(g.nx) * g.ny;
    return static_cast<unsigned>(std::min((cells + 63) / 64, RELAX_MAX_BLOCKS));
}

// the lane offset is 32 bits wide
bool relax_ok(const EnsGeom& g, int M) { return M >= 2 && M <= ASSIM_MAX_MEMBERS && g.slab <= 0x7fffffffL; }

}  // namespace

hipError_t ens_launch_relax_capture(const EnsGeom& g, const double* f, int forecast, int truth_member, double* sb,
                                    hipStream_t st) {
    if (!relax_ok(g, forecast)) return hipErrorInvalidValue;
    return for_step(forecast, [&](auto s) {
        hipLaunchKernelGGL(k_relax_capture<decltype(s)::value>, dim3(relax_blocks(g)), dim3(64), 0, st, f, g.nx, g.ny,
                           g.pitch, g.slab, forecast, truth_member, sb);
        return hipGetLastError();
    });
}

hipError_t ens_launch_relax_spread(const EnsGeom& g, double* f, int forecast, int truth_member, double alpha,
                                   const double* sb, double* factor, hipStream_t st) {
    if (!relax_ok(g, forecast)) return hipErrorInvalidValue;
    return for_step(forecast, [&](auto s) {
        hipLaunchKernelGGL(k_relax_spread<decltype(s)::value>, dim3(relax_blocks(g)), dim3(64), 0, st, f, g.nx, g.ny,
                           g.pitch, g.slab, forecast, truth_member, alpha, sb, factor);
        return hipGetLastError();
    });
}

hipError_t ens_launch_relax_pert(const EnsGeom& g, double* f, const double* fb, int forecast, int truth_member,
                                 double alpha, hipStream_t st) {
    if (!relax_ok(g, forecast)) return hipErrorInvalidValue;
    return for_step(forecast, [&](auto s) {
        hipLaunchKernelGGL(k_relax_pert<decltype(s)::value>, dim3(relax_blocks(g)), dim3(64), 0, st, f, fb, g.nx, g.ny,
                           g.pitch, g.slab, forecast, truth_member, alpha);
        return hipGetLastError();
    });
}

}  // namespace csim
