// espace_cell.hpp — a cell's perturbations, held and applied: what k_espace_apply (ensemble_space.hip) and k_letkf_cells
// (ensemble_letkf.hip) share, said once, so that the project, the transform and the LETKF's cell pass keep the bits they
// promise to agree on.  One cell per lane; p_k = x_k - m, m the cell's mean (mean_regs' running sum) when centered, +0
// otherwise.  Two forms, as everywhere behind for_step:
//   P > 0  one wave; the lane's p_k in registers x[P].  Loads beyond M load member M - 1 again, the sums skip them.
//   P = 0  CELL_WAVES waves share 64 cells in LDS as held[k * 64 + lane] (512 B per member) and divide the outputs among
//          them, so that the tile keeps four waves busy instead of one.  x is a dummy of one element.
// Every product and every sum is one rounded fp64 operation, no FMA contraction.  The vectors and matrices are read with
// wave-uniform indices, so their loads are scalar.  Every piece is force-inlined into its kernel or is macro text.
#pragma once

#include "ensemble_cell.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr int CELL_RB = 4;     // outputs r that share one pass over k
constexpr int CELL_WAVES = 4;  // LDS form: waves that share 64 cells, each taking every fourth group of outputs

// Holds p_k of the cell at p (its address in member 0) and returns m.  P = 0: the waves load the members together, every
// wave sums the mean of its lane's cell (the same bits in each), and the waves subtract it from a quarter of the members
// each; every wave of the workgroup must call, and the tile is the caller's to free with a barrier before the next cells.
template <int P>
__device__ __forceinline__ double cell_hold(const double* __restrict__ p, long slab, int M, int t, bool centered, int lane,
                                            int wave, double (&x)[P > 0 ? P : 1], double* __restrict__ held) {
    double m = 0.0;
    if constexpr (P > 0) {
#pragma unroll
        for (int k = 0; k < P; ++k) x[k] = p[static_cast<size_t>(forecast_member(min(k, M - 1), t)) * slab];
        if (centered) {
            m = mean_regs<P>(x, M);
#pragma unroll
            for (int k = 0; k < P; ++k) x[k] = x[k] - m;
        }
    } else {
#pragma unroll 8
        for (int k = wave; k < M; k += CELL_WAVES) held[k * 64 + lane] = p[static_cast<size_t>(forecast_member(k, t)) * slab];
        __syncthreads();
        if (centered) {
            double s = 0.0;
#pragma unroll 8
            for (int k = 0; k < M; ++k) s = s + held[k * 64 + lane];
            m = s / static_cast<double>(M);
            __syncthreads();  // every wave has read the members it did not load before any is replaced
#pragma unroll 8
            for (int k = wave; k < M; k += CELL_WAVES) held[k * 64 + lane] = held[k * 64 + lane] - m;
            __syncthreads();
        }
    }
    return m;
}

// sum_k p_k v[k], a running sum from +0 in member order
template <int P>
__device__ __forceinline__ double cell_dot(const double (&x)[P > 0 ? P : 1], const double* __restrict__ held, int lane,
                                           int M, const double* __restrict__ v) {
    double d = 0.0;
    if constexpr (P > 0) {
#pragma unroll
        for (int k = 0; k < P; ++k)
            if (k < M) d = d + x[k] * v[k];
    } else {
#pragma unroll 4
        for (int k = 0; k < M; ++k) d = d + held[k * 64 + lane] * v[k];
    }
    return d;
}

// s[u] += p_k W[k * ld + rr[u]] in member order: one pass over k feeds the CELL_RB outputs, independent chains.  The LDS
// form is a function; the register form is macro text, like CSIM_LOAD_TILE and for its reason: as a function it leaves
// k_espace_apply<64, false> with six more spilled SGPRs and so one more VGPR
__device__ __forceinline__ void cell_apply_lds(const double* __restrict__ held, int lane, int M,
                                               const double* __restrict__ W, int ld, const int (&rr)[CELL_RB],
                                               double (&s)[CELL_RB]) {
#pragma unroll 4
    for (int k = 0; k < M; ++k) {
        const double pk = held[k * 64 + lane];
#pragma unroll
        for (int u = 0; u < CELL_RB; ++u) s[u] = s[u] + pk * W[static_cast<size_t>(k) * ld + rr[u]];
    }
}

#define CSIM_CELL_APPLY(P, x, held, lane, M, W, ld, rr, s)                                                             \
    if constexpr ((P) > 0) {                                                                                          \
        _Pragma("unroll") for (int k_ = 0; k_ < (P); ++k_) if (k_ < (M)) {                                            \
            _Pragma("unroll") for (int u_ = 0; u_ < CELL_RB; ++u_)                                                    \
                (s)[u_] = (s)[u_] + (x)[k_] * (W)[static_cast<size_t>(k_) * (ld) + (rr)[u_]];                         \
        }                                                                                                             \
    } else {                                                                                                          \
        cell_apply_lds(held, lane, M, W, ld, rr, s);                                                                  \
    }

}  // namespace

}  // namespace csim
