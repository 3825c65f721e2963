// ensemble_cell.hpp — one cell of an ensemble across its members: what the per-cell kernels of ensemble_stats,
// _quantiles, _verify, _assim, _relax and _impact .hip share, said once.  Needs only the slab layout of ensemble.hpp.  Every
// device piece is force-inlined into its kernel (the tile's loader is a macro); the host pieces choose a kernel's
// instantiation, size its tile and raise its dynamic LDS limit.
//
// Forecast member k of M is member forecast_member(k, t) of the ensemble: the truth member t is stepped over (t = B:
// none skipped).  A cell of member m is f[m * slab + off], a wave-uniform member base plus one 32-bit lane offset.
// The diagnostics number the dense layout (ny+2) x (nx+2), ghost ring included, c = j (nx+2) + i (dense_cell): lanes
// past the end load the last cell and store nothing, so no load is predicated.  The analysis numbers the interior,
// e = (j - 1) nx + (i - 1) (cell_of).  Either way lanes follow i, so each member's load coalesces.
//
// Sums over the members of a cell are running sums from +0 in member order, one rounding per operation, no FMA
// contraction, / IEEE fp64: m = sum x_k / M, v = sum (x_k - m)^2 / (M - 1), which the numpy restatements repeat bit
// for bit.  Two forms, chosen by for_step:
//   P > 0 (M <= P, P = 4, 8, 16, 32, 48, 64)  a lane reads its cell of every member once into registers
//                 (load_members), holds them across the sums (mean_regs, var_regs) and writes each at most once.
//                 Loads beyond M load member M - 1 again instead of branching per member; the sums skip those.
//   P = 0 (M > 64) one pass over the members per sum (mean_mem, var_mem); they stay in L2 between the passes.  The
//                 loops are unrolled by 8 so that eight loads are in flight before the running sum takes them in order.
// Order statistics (the networks of ensemble_sort.hpp) have two forms as well, chosen by for_sort_form from the number
// n of values to sort:
//   lane form (n <= 64)  one cell per lane, P = 2^ceil(log2 n) values per lane in registers, padded with +inf.
//   wave form (64 < n <= SORT_MAX_VALUES)  one cell per wave, E = P / 64 values per lane.  Four waves load a tile of
//                 ct consecutive cells x all B members into LDS (CSIM_LOAD_TILE), cell-major with the odd row stride
//                 B | 1, so that both the tile's stores and a wave's reads down one cell's members are free of bank
//                 conflicts.  sort_tile sizes it: ct = 16, halved down to 4 while the tile and whatever else the
//                 kernel keeps in dynamic LDS exceed 64 KiB (two workgroups, eight waves, per CU).
#pragma once

#include <type_traits>

#include "ensemble.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

__device__ __forceinline__ int forecast_member(int k, int t) { return k + (k >= t); }

// cell (i, j) of a member: its offset from the buffer's row j = 0, and its address in member 0
__device__ __forceinline__ unsigned cell_off(int i, int j, int pitch) {
    return static_cast<unsigned>(j * pitch + (LPAD - 1) + i);
}
template <class T>
__device__ __forceinline__ T* cell_ptr(T* f, int i, int j, int pitch) {
    return f + static_cast<ptrdiff_t>(j) * pitch + (LPAD - 1) + i;
}

// interior cell e = (j - 1) nx + (i - 1).  Its offset is spelled out (through cell_off k_relax_pert compiles to other
// code) and in unsigned arithmetic: k_assim_inflate, which does not bound a slab to 2^31 doubles, uses i and j alone
struct Cell {
    unsigned off;
    int i, j;
};
__device__ __forceinline__ Cell cell_of(long e, int nx, int pitch) {
    const int j0 = static_cast<int>(e / nx);
    const int i = static_cast<int>(e - static_cast<long>(j0) * nx) + 1;
    return {static_cast<unsigned>(j0 + 1) * pitch + (LPAD - 1) + i, i, j0 + 1};
}

// dense cell c = j nx2 + i, clamped to the last one (the caller stores only where c < ncells)
struct DenseCell {
    int c, i, j;
};
__device__ __forceinline__ DenseCell dense_cell(int c, int nx2, int ncells) {
    const int cc = min(c, ncells - 1);
    const int j = cc / nx2;
    return {cc, cc - j * nx2, j};
}

template <int P>
__device__ __forceinline__ void load_members(const double* __restrict__ f, long slab, unsigned off, int M, int t,
                                             double (&x)[P]) {
#pragma unroll
    for (int k = 0; k < P; ++k) x[k] = f[static_cast<size_t>(forecast_member(min(k, M - 1), t)) * slab + off];
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

// (f may be the cell's own address in member 0 and off = 0: kernels that do not bound a slab to 32-bit offsets)
__device__ __forceinline__ double mean_mem(const double* __restrict__ f, long slab, unsigned off, int M, int t) {
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < M; ++k) s = s + f[static_cast<size_t>(forecast_member(k, t)) * slab + off];
    return s / static_cast<double>(M);
}

__device__ __forceinline__ double var_mem(const double* __restrict__ f, long slab, unsigned off, int M, int t,
                                          double m) {
    double q = 0.0;
#pragma unroll 8
    for (int k = 0; k < M; ++k) {
        const double d = f[static_cast<size_t>(forecast_member(k, t)) * slab + off] - m;
        q = q + d * d;
    }
    return q / static_cast<double>(M - 1);
}

// c = sum (x_k - xbar) h_k, h wave-uniform (LDS): the covariance of a cell with an observation, before its / (M - 1)
template <int P>
__device__ __forceinline__ double cov_regs(const double (&x)[P], int M, double xbar, const double* h) {
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k)
        if (k < M) c = c + (x[k] - xbar) * h[k];
    return c;
}

// (p: the cell's own address in member 0.)  U: the loop's unroll count.  The impact takes the 8 of the other P = 0
// loops; the update, which writes the members afterwards, keeps 1: with 8 it needs 66 VGPRs, not 48
template <int U>
__device__ __forceinline__ double cov_mem(const double* p, long slab, int M, int t, double xbar, const double* h) {
    double c = 0.0;
#pragma unroll U
    for (int k = 0; k < M; ++k) c = c + (p[static_cast<ptrdiff_t>(forecast_member(k, t)) * slab] - xbar) * h[k];
    return c;
}

// m and v of M values that are already in LDS, every lane the same
__device__ __forceinline__ void mv(const double* x, int M, double& m, double& v) {
    double s = 0.0;
    for (int k = 0; k < M; ++k) s = s + x[k];
    m = s / static_cast<double>(M);
    double q = 0.0;
    for (int k = 0; k < M; ++k) {
        const double d = x[k] - m;
        q = q + d * d;
    }
    v = q / static_cast<double>(M - 1);
}

// 256 threads: cells c0 .. c0 + ct - 1 (ct a power of two, clamped to the last cell) of all `members` members into
// held[cell][stride].  Thread tid loads cell tid % ct of members tid / ct, + 256 / ct, ...: ct consecutive cells per
// member load, eight loads in flight.  The caller puts the barriers around it.  A macro like CSIM_SORT_LANE, and for
// its reason: as a function the same text leaves the kernels around it with other registers.
#define CSIM_LOAD_TILE(f, nx2, ncells, pitch, slab, members, ct, stride, c0, tid, held)                               \
    {                                                                                                                 \
        const int cl_ = (tid) & ((ct) - 1);                                                                           \
        const DenseCell d_ = dense_cell((c0) + cl_, nx2, ncells);                                                     \
        const double* __restrict__ p_ = cell_ptr(f, d_.i, d_.j, pitch);                                               \
        const int step_ = 256 / (ct);                                                                                 \
        double* row_ = (held) + cl_ * (stride);                                                                       \
        int m_ = (tid) / (ct);                                                                                        \
        for (; m_ + 7 * step_ < (members); m_ += 8 * step_) {                                                         \
            double x_[8];                                                                                             \
            _Pragma("unroll") for (int u_ = 0; u_ < 8; ++u_)                                                          \
                x_[u_] = p_[static_cast<ptrdiff_t>(m_ + u_ * step_) * (slab)];                                        \
            _Pragma("unroll") for (int u_ = 0; u_ < 8; ++u_) row_[m_ + u_ * step_] = x_[u_];                          \
        }                                                                                                             \
        for (; m_ < (members); m_ += step_) row_[m_] = p_[static_cast<ptrdiff_t>(m_) * (slab)];                       \
    }

constexpr int SORT_LDS_BUDGET = 64 * 1024;
constexpr int SORT_TILE_MAX = 16;                    // cells per tile, at most
constexpr int SORT_MAX_VALUES = QUANT_MAX_MEMBERS;   // the largest network: 64 values per lane of a wave
static_assert(VERIFY_MAX_MEMBERS <= SORT_MAX_VALUES, "for_sort_form refuses what the verification accepts");

// the tile of `members` members for a kernel that keeps `extra` more bytes behind it; lds: tile and extra together
struct SortTile {
    int ct, stride;
    size_t lds;
};
inline SortTile sort_tile(int members, size_t extra) {
    const int stride = members | 1;
    int ct = SORT_TILE_MAX;
    while (ct > 4 && static_cast<size_t>(ct) * stride * sizeof(double) + extra > SORT_LDS_BUDGET) ct >>= 1;
    return {ct, stride, static_cast<size_t>(ct) * stride * sizeof(double) + extra};
}

template <int P>
using Step = std::integral_constant<int, P>;

// launch(Step<P>) with the register step of M, or P = 0 above 64 members
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

// lane(Step<P>) with the lane form's P for n values, or wave(Step<E>) with the wave form's E
template <class L, class W>
hipError_t for_sort_form(int n, L&& lane, W&& wave) {
    if (n <= 1) return lane(Step<1>{});
    if (n <= 2) return lane(Step<2>{});
    if (n <= 4) return lane(Step<4>{});
    if (n <= 8) return lane(Step<8>{});
    if (n <= 16) return lane(Step<16>{});
    if (n <= 32) return lane(Step<32>{});
    if (n <= 64) return lane(Step<64>{});
    if (n <= 128) return wave(Step<2>{});
    if (n <= 256) return wave(Step<4>{});
    if (n <= 512) return wave(Step<8>{});
    if (n <= 1024) return wave(Step<16>{});
    if (n <= 2048) return wave(Step<32>{});
    if (n <= SORT_MAX_VALUES) return wave(Step<64>{});
    return hipErrorInvalidValue;  // the host refuses these first
}

// kernel K may be launched with up to `bytes` of dynamic LDS: asked of the runtime once per kernel, the answer kept
template <auto K>
hipError_t dynamic_lds_once(size_t bytes) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(K),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       static_cast<int>(bytes));
    return attr;
}

}  // namespace

}  // namespace csim
