// ensemble_relax.hip — the relaxation inflation of csim_ensemble_prior_capture / csim_ensemble_relax (host side in
// ensemble_da.cpp): relaxation to prior spread (RTPS) and to prior perturbations (RTPP), the block in csim.h.  Needs
// only the slab layout of ensemble.hpp.
//
// Every kernel: one lane per interior cell, numbered row by row, lanes along i, so each member's load coalesces.
// Forecast member k is member k + (k >= t) of the ensemble (t = B: none skipped).  Two forms, as k_assim_update:
//   P > 0 (M <= P, P = 4, 8, 16, 32, 48, 64)  a lane reads its cell of every member once into registers, holds them
//                 across both sums and writes each at most once.  Loads beyond M load member M - 1 again instead of
//                 branching per member (the sums skip those); a member is addressed as a wave-uniform member base plus
//                 one 32-bit lane offset.
//   P = 0 (M > 64) one pass over the members per sum and one for the update; they stay in L2 between the passes.  The
//                 loops are unrolled by 8 so that eight loads are in flight before the running sum takes them in order.
//   k_relax_capture  sb = sqrt(v) of mv(x), one store per cell
//   k_relax_spread   sa = sqrt(v) of mv(x), fac = sa > 0 ? alpha ((sb - sa) / sa) : +0; where fac == 0 nothing is
//                    written (outside every observation window the analysis left the bits alone, so fac is exactly +0)
//   k_relax_pert     the means of x and of the captured xb, then the update.  The register form holds x_k only: xb_k is
//                    read for its mean and read again (from L2) for the update, which keeps P = 64 at the registers of
//                    k_relax_spread instead of twice as many.
// Every sum is a running sum from +0 in member order, without FMA contraction; / and sqrt are IEEE fp64 (no
// fast-math), so the numpy restatement (tests/relax_restatement.py) gives the same bits.  Only interior cells of the
// forecast members are written; ghost rings, member t and the other ping-pong buffer are never touched.
#include <algorithm>
#include <type_traits>

#include "ensemble.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr long RELAX_MAX_BLOCKS = 1L << 20;  // larger fields loop

// the cell's offset in a member's slab (from the buffer's row j = 0), and its interior index e = (j - 1) nx + (i - 1)
struct Cell {
    unsigned off;
    int i, j;
};
__device__ __forceinline__ Cell cell_of(long e, int nx, int pitch) {
    const int j0 = static_cast<int>(e / nx);
    const int i = static_cast<int>(e - static_cast<long>(j0) * nx) + 1;
    return {static_cast<unsigned>((j0 + 1) * pitch + (LPAD - 1) + i), i, j0 + 1};
}

template <int P>
__device__ __forceinline__ void load_members(const double* __restrict__ f, long slab, unsigned off, int M, int t,
                                             double (&x)[P]) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int kk = min(k, M - 1);
        x[k] = f[static_cast<size_t>(kk + (kk >= t)) * slab + off];
    }
}

template <int P>
__device__ __forceinline__ double mean_regs(const double (&x)[P], int M) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k)
        if (k < M) s = s + x[k];
    return s / static_cast<double>(M);
}

template <int P>
__device__ __forceinline__ double var_regs(const double (&x)[P], int M, double m) {
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k)
        if (k < M) {
            const double d = x[k] - m;
            q = q + d * d;
        }
    return q / static_cast<double>(M - 1);
}

__device__ __forceinline__ double mean_mem(const double* __restrict__ f, long slab, unsigned off, int M, int t) {
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < M; ++k) s = s + f[static_cast<size_t>(k + (k >= t)) * slab + off];
    return s / static_cast<double>(M);
}

__device__ __forceinline__ double var_mem(const double* __restrict__ f, long slab, unsigned off, int M, int t,
                                          double m) {
    double q = 0.0;
#pragma unroll 8
    for (int k = 0; k < M; ++k) {
        const double d = f[static_cast<size_t>(k + (k >= t)) * slab + off] - m;
        q = q + d * d;
    }
    return q / static_cast<double>(M - 1);
}

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
                    if (k < M) f[static_cast<size_t>(k + (k >= t)) * slab + c.off] = x[k] + fac * (x[k] - m2);
            }
        } else {
            const double m = mean_mem(f, slab, c.off, M, t);
            const double sa = sqrt(var_mem(f, slab, c.off, M, t, m));
            const double fac = sa > 0.0 ? alpha * ((b - sa) / sa) : 0.0;
            if (factor) factor[static_cast<size_t>(c.j) * (nx + 2) + c.i] = fac;
            if (!(fac == 0.0)) {
#pragma unroll 8
                for (int k = 0; k < M; ++k) {
                    const size_t o = static_cast<size_t>(k + (k >= t)) * slab + c.off;
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
                    const size_t o = static_cast<size_t>(k + (k >= t)) * slab + c.off;
                    f[o] = x[k] + alpha * ((fb[o] - mb) - (x[k] - m));
                }
        } else {
            const double m = mean_mem(f, slab, c.off, M, t);
#pragma unroll 8
            for (int k = 0; k < M; ++k) {
                const size_t o = static_cast<size_t>(k + (k >= t)) * slab + c.off;
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

// calls launch(Step<P>) with the register step of M, or P = 0 above 64 members
template <int P>
using Step = std::integral_constant<int, P>;
template <class F>
hipError_t for_step(int M, F&& launch) {
    if (M <= 4) return launch(Step<4>{});
    if (M <= 8) return launch(Step<8>{});
    if (M <= 16) return launch(Step<16>{});
    if (M <= 32) return launch(Step<32>{});
    if (M <= 48) return launch(Step<48>{});
    if (M <= 64) return launch(Step<64>{});
    return launch(Step<0>{});
}

}  // namespace

hipError_t ens_launch_relax_capture(const EnsGeom& g, const double* f, int forecast, int truth_member, double* sb,
                                    hipStream_t st) {
    if (!relax_ok(g, forecast)) return hipErrorInvalidValue;
    return for_step(forecast, [&](auto s) {
        constexpr int P = decltype(s)::value;
        hipLaunchKernelGGL(k_relax_capture<P>, dim3(relax_blocks(g)), dim3(64), 0, st, f, g.nx, g.ny, g.pitch, g.slab,
                           forecast, truth_member, sb);
        return hipGetLastError();
    });
}

hipError_t ens_launch_relax_spread(const EnsGeom& g, double* f, int forecast, int truth_member, double alpha,
                                   const double* sb, double* factor, hipStream_t st) {
    if (!relax_ok(g, forecast)) return hipErrorInvalidValue;
    return for_step(forecast, [&](auto s) {
        constexpr int P = decltype(s)::value;
        hipLaunchKernelGGL(k_relax_spread<P>, dim3(relax_blocks(g)), dim3(64), 0, st, f, g.nx, g.ny, g.pitch, g.slab,
                           forecast, truth_member, alpha, sb, factor);
        return hipGetLastError();
    });
}

hipError_t ens_launch_relax_pert(const EnsGeom& g, double* f, const double* fb, int forecast, int truth_member,
                                 double alpha, hipStream_t st) {
    if (!relax_ok(g, forecast)) return hipErrorInvalidValue;
    return for_step(forecast, [&](auto s) {
        constexpr int P = decltype(s)::value;
        hipLaunchKernelGGL(k_relax_pert<P>, dim3(relax_blocks(g)), dim3(64), 0, st, f, fb, g.nx, g.ny, g.pitch, g.slab,
                           forecast, truth_member, alpha);
        return hipGetLastError();
    });
}

}  // namespace csim
