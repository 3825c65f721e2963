// ensemble_space.hip — the ensemble-space primitives of csim_ensemble_gram, _project and _transform (host side in
// ensemble_space.cpp; the definitions are the block in csim.h).  Needs only the slab layout of ensemble.hpp.
//
// p_k of a cell: x_k less the cell's mean m = (running sum of x_k from +0 in member order) / M when centered, x_k
// otherwise.  Every product and every sum is one rounded fp64 operation, no FMA contraction.
//
// Gram, two kernels:
//   k_gram_partial  Workgroup (g, y) of 256 lanes serves class g: the segments g, g + Gc, ... of 64 interior cells.  A
//                   segment's perturbations staged in LDS as [cell][member] (gram_stage_cells), the walk over them,
//                   the lanes' pairs and the class's partial (GramTile) are gram_tile.hpp, the plan is gram_plan.hpp.
//   k_gram_fold     entry (a, b), a <= b, folded over the classes (gram_fold_entry); written to G[a][b] and G[b][a].
// Project / transform, one kernel template k_espace_apply<P, XFORM>: one cell per lane, its p_k held and applied by
// espace_cell.hpp, in registers (P > 0, the steps of for_step) or in LDS (P = 0: M > 64, or project_form 1).  All M
// values of a cell are held before any is stored, so the transform may write the members it read.
#include <algorithm>

#include "espace_cell.hpp"
#include "gram_tile.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr long ESPACE_MAX_BLOCKS = 1L << 20;  // larger fields loop

template <int NB>
__global__ __launch_bounds__(GRAM_THREADS) void k_gram_partial(const double* __restrict__ f, int nx, long cells,
                                                               long nseg, int pitch, long slab, int M, int t,
                                                               int centered, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) double held[];  // [64][stride], then the 64 means
    GramTile<NB> tile;
    tile.init(M);
    for (long q = blockIdx.x; q < nseg; q += gridDim.x) {
        const long e0 = q * GRAM_SEG;
        const int nc = static_cast<int>(min(static_cast<long>(GRAM_SEG), cells - e0));
        gram_stage_cells(f, nx, pitch, slab, M, t, centered, e0, nc, held);
        tile.walk(held, gram_stride(M), nc);
        __syncthreads();
    }
    tile.store(partial + static_cast<size_t>(blockIdx.x) * gram_pairs(M), M);
}

// grid (ceil(M / 64), M): row a = blockIdx.y, column b
__global__ __launch_bounds__(64) void k_gram_fold(const double* __restrict__ partial, int classes, int M,
                                                  double* __restrict__ G) {
    const int a = blockIdx.y, b = blockIdx.x * 64 + threadIdx.x;
    if (b < a || b >= M) return;
    const double s = gram_fold_entry(partial + gram_packed(a, b, M), classes, gram_pairs(M));
    G[static_cast<size_t>(a) * M + b] = s;
    G[static_cast<size_t>(b) * M + a] = s;
}

// XFORM = false: project; cells are the dense cells of (ny+2) x (nx+2), out gets K fields.
// XFORM = true: transform; cells are the interior cells, K = M, the members are written in place.
// P > 0: one wave per workgroup.  P = 0: CELL_WAVES waves, wave w computes the outputs r of groups w, w + CELL_WAVES, ...
template <int P, bool XFORM>
__global__ __launch_bounds__(P > 0 ? 64 : 64 * CELL_WAVES) void k_espace_apply(
    double* __restrict__ f, int nx, int ny, int pitch, long slab, int M, int t, int centered, int K,
    const double* __restrict__ W, const double* __restrict__ wbar, double* __restrict__ out, const int* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(16))) double held[];  // P = 0: [M][64]
    // the transform of a device ETKF obeys the status its weights kernel left: the whole grid returns at once
    if (XFORM && gate && (*gate == ETKF_NONFINITE || *gate == ETKF_SKIP)) return;
    constexpr int NW = P > 0 ? 1 : CELL_WAVES;
    // the register form is one wave: `wave` is a constant 0 there, so the loop over the outputs keeps no state for it
    const int lane = threadIdx.x & 63, wave = P > 0 ? 0 : threadIdx.x >> 6;
    const int nx2 = nx + 2;
    const long cells = XFORM ? static_cast<long>(nx) * ny : static_cast<long>(nx2) * (ny + 2);
    const long rounded = (cells + 63) / 64 * 64;  // whole waves: a lane past the end works on the last cell, stores nothing
    for (long e = static_cast<long>(blockIdx.x) * 64 + lane; e < rounded; e += static_cast<long>(gridDim.x) * 64) {
        const bool valid = e < cells;
        const long ec = valid ? e : cells - 1;
        double* __restrict__ p;
        if (XFORM) {
            p = f + static_cast<size_t>(cell_of(ec, nx, pitch).off);
        } else {
            const int j = static_cast<int>(ec / nx2);
            p = cell_ptr(f, static_cast<int>(ec - static_cast<long>(j) * nx2), j, pitch);
        }
        double x[P > 0 ? P : 1];
        const double m = cell_hold<P>(p, slab, M, t, centered != 0, lane, wave, x, held);
        double mp = m;
        if (XFORM && wbar) mp = m + cell_dot<P>(x, held, lane, M, wbar);
        for (int r0 = CELL_RB * wave; r0 < K; r0 += CELL_RB * NW) {
            int rr[CELL_RB];
            double s[CELL_RB];
#pragma unroll
            for (int u = 0; u < CELL_RB; ++u) rr[u] = min(r0 + u, K - 1), s[u] = 0.0;
            CSIM_CELL_APPLY(P, x, held, lane, M, W, K, rr, s)
#pragma unroll
            for (int u = 0; u < CELL_RB; ++u) {
                if (r0 + u >= K || !valid) continue;
                if (XFORM)
                    p[static_cast<size_t>(forecast_member(r0 + u, t)) * slab] = centered ? mp + s[u] : s[u];
                else
                    out[static_cast<size_t>(r0 + u) * cells + e] = s[u];
            }
        }
        if constexpr (P == 0) __syncthreads();  // the tile is free for the next cells
    }
}

template <int NB>
hipError_t launch_gram(const EnsGeom& g, const double* f, int M, int t, bool centered, double* partial, double* G,
                       hipStream_t st) {
    const long cells = static_cast<long>(g.nx) * g.ny;
    const int classes = gram_classes(M, cells);
    const size_t lds = sizeof(double) * gram_lds_doubles(M);
    const hipError_t attr = dynamic_lds_once<k_gram_partial<NB>>(sizeof(double) * gram_lds_doubles(ESPACE_MAX_MEMBERS));
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(k_gram_partial<NB>, dim3(classes, gram_shares(M, NB)), dim3(GRAM_THREADS), lds, st, f, g.nx,
                       cells, gram_segments(cells), g.pitch, g.slab, M, t, centered ? 1 : 0, partial);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(k_gram_fold, dim3((M + 63) / 64, M), dim3(64), 0, st, partial, classes, M, G);
    return hipGetLastError();
}

unsigned apply_blocks(long cells) { return static_cast<unsigned>(std::min((cells + 63) / 64, ESPACE_MAX_BLOCKS)); }

template <bool XFORM>
hipError_t launch_apply(const EnsGeom& g, double* f, int M, int t, bool centered, int K, const double* W,
                        const double* wbar, double* out, int form, hipStream_t st, const int* gate = nullptr) {
    const long cells = XFORM ? static_cast<long>(g.nx) * g.ny : static_cast<long>(g.nx + 2) * (g.ny + 2);
    auto launch = [&](auto s) {
        constexpr int P = decltype(s)::value;
        const size_t lds = P > 0 ? 0 : sizeof(double) * 64 * static_cast<size_t>(M);
        if (P == 0) {
            const hipError_t attr =
                dynamic_lds_once<k_espace_apply<P, XFORM>>(sizeof(double) * 64 * ESPACE_MAX_MEMBERS);
            if (attr != hipSuccess) return attr;
        }
        hipLaunchKernelGGL((k_espace_apply<P, XFORM>), dim3(apply_blocks(cells)), dim3(P > 0 ? 64 : 64 * CELL_WAVES), lds, st, f, g.nx, g.ny,
                           g.pitch, g.slab, M, t, centered ? 1 : 0, K, W, wbar, out, gate);
        return hipGetLastError();
    };
    if (form == 1) return launch(Step<0>{});
    return for_step(M, launch);
}

bool espace_ok(int M, int form, int forms) { return M >= 1 && M <= ESPACE_MAX_MEMBERS && form >= 0 && form <= forms; }

}  // namespace

hipError_t ens_launch_gram(const EnsGeom& g, const double* f, int forecast, int truth_member, bool centered,
                           double* partial, double* G, int form, hipStream_t st) {
    if (!espace_ok(forecast, form, GRAM_FORMS)) return hipErrorInvalidValue;
    return for_gram_form(form, forecast, [&](auto nb) {
        return launch_gram<decltype(nb)::value>(g, f, forecast, truth_member, centered, partial, G, st);
    });
}

hipError_t ens_launch_project(const EnsGeom& g, const double* f, int forecast, int truth_member, bool centered, int K,
                              const double* W, double* out, int form, hipStream_t st) {
    if (!espace_ok(forecast, form, PROJECT_FORMS) || K < 1 || K > forecast) return hipErrorInvalidValue;
    return launch_apply<false>(g, const_cast<double*>(f), forecast, truth_member, centered, K, W, nullptr, out, form,
                               st);
}

hipError_t ens_launch_transform(const EnsGeom& g, double* f, int forecast, int truth_member, bool centered,
                                const double* W, const double* wbar, int form, hipStream_t st, const int* gate) {
    if (!espace_ok(forecast, form, PROJECT_FORMS) || (wbar && !centered)) return hipErrorInvalidValue;
    return launch_apply<true>(g, f, forecast, truth_member, centered, forecast, W, wbar, nullptr, form, st, gate);
}

}  // namespace csim
