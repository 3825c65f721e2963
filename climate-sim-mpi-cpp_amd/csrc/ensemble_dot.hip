// ensemble_dot.hip — the kernels of csim_ensemble_dot and csim_ensemble_obs_impact_global (host side in
// ensemble_space.cpp and ensemble_obs_impact.cpp; the definitions are in csim.h).  Needs only the slab layout of ensemble.hpp.
// All three kernels only read the members.
//
// p_k of a cell as in ensemble_space.hip.  Every product and every sum is one rounded fp64 operation, no FMA contraction.
//
// Dot, out[k][r] = sum over the interior of p_k f_r, two kernels with the plan of the Gram sum (gram_plan.hpp: segments
// of 64 interior cells, gram_classes(M, cells) classes):
//   k_dot_partial  Workgroup g of 256 lanes serves class g.  A segment's perturbations are staged in LDS as
//                  [cell][member] by the routine that k_gram_partial calls (gram_stage_cells of gram_tile.hpp), and
//                  beside them, its own, the K field values of each cell as [cell][field] (+0 from field K up).  The
//                  M x K sums are cut into blocks of 4 x 4, DotTile, over the rectangle of gram_plan.hpp (dot_owned:
//                  one workgroup per class holds all blocks, so there is one geometry); a row's step onto a block is
//                  gram_block_step, GramTile's.  A wave whose lanes own no block only helps staging.  The walk adds a
//                  segment's cells in order and the sums are carried from segment to segment of the class: the order of
//                  each sum is that of the cells.
//   k_dot_fold     entry (k, r) folded over the classes in class order (gram_fold_entry).
// With K = 1 and M = 64 only 16 lanes walk, and the walk is short next to the staging: at 37 KiB of LDS four
// workgroups share a CU and one's staging runs beside another's walk.
//
// Global impact, one kernel:
//   k_obs_impact_global  one lane per plan position q, one wave per 64 of them.  The wave stages a_{q,k} of its used
//                  observations through LDS, 64 members at a time: row by row with coalesced loads, rows 65 doubles
//                  apart, so that lane q's reads along its row meet no other lane's bank.  g is staged beside them and
//                  broadcast.  Each lane sums c = c + a_k g_k in member order, carried over the tiles of 64 members.
//                  Nothing of an observation that was not used is read; it gets +0.
#include <algorithm>

#include "gram_tile.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

struct DotTile {
    int im, ik;    // member block, field block
    bool mine;
    bool wave_on;  // false: this wave only helps staging
    double acc[GRAM_TB * GRAM_TB];

    __device__ __forceinline__ void init(int M, int K) {
        const DotOwned o = dot_owned(threadIdx.x, M, K);
        im = o.im, ik = o.ik, mine = o.mine;
        wave_on = dot_wave_on(threadIdx.x, M, K);
#pragma unroll
        for (int v = 0; v < GRAM_TB * GRAM_TB; ++v) acc[v] = 0.0;
    }

    // the cells 0 .. nc - 1 of a segment, in order
    __device__ __forceinline__ void walk(const double* __restrict__ held, int stride, const double* __restrict__ fl,
                                         int fstride, int nc) {
        if (!wave_on) return;
#pragma unroll 2
        for (int cc = 0; cc < nc; ++cc)
            gram_block_step(held + cc * stride + GRAM_TB * im, fl + cc * fstride + GRAM_TB * ik, acc);
    }

    // the class's partial, M x K row-major
    __device__ __forceinline__ void store(double* __restrict__ class_partial, int M, int K) const {
        if (!mine) return;
#pragma unroll
        for (int i = 0; i < GRAM_TB; ++i)
#pragma unroll
            for (int j = 0; j < GRAM_TB; ++j) {
                const int k = GRAM_TB * im + i, r = GRAM_TB * ik + j;
                if (k < M && r < K) class_partial[static_cast<size_t>(k) * K + r] = acc[i * GRAM_TB + j];
            }
    }
};

// fields: K fields of `cells` values, interior cell e of field r at r cells + e
__global__ __launch_bounds__(GRAM_THREADS) void k_dot_partial(const double* __restrict__ f, int nx, long cells,
                                                              long nseg, int pitch, long slab, int M, int t,
                                                              int centered, int K, const double* __restrict__ fields,
                                                              double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) double held[];  // [64][stride], the 64 means, [64][fstride]
    const int fstride = dot_fstride(K), kpad = gram_nblk(K) * GRAM_TB;
    double* __restrict__ fl = held + gram_lds_doubles(M);
    DotTile tile;
    tile.init(M, K);

    const int c = threadIdx.x & 63, kq = threadIdx.x >> 6;
    double* __restrict__ frow = fl + c * fstride;
    for (long q = blockIdx.x; q < nseg; q += gridDim.x) {
        const long e0 = q * GRAM_SEG;
        const int nc = static_cast<int>(min(static_cast<long>(GRAM_SEG), cells - e0));
        if (c < nc) {
            for (int r = kq; r < K; r += 4) frow[r] = fields[static_cast<size_t>(r) * cells + (e0 + c)];
            for (int r = K + kq; r < kpad; r += 4) frow[r] = 0.0;
        }
        gram_stage_cells(f, nx, pitch, slab, M, t, centered, e0, nc, held);
        tile.walk(held, gram_stride(M), fl, fstride, nc);
        __syncthreads();
    }
    tile.store(partial + static_cast<size_t>(blockIdx.x) * M * K, M, K);
}

__global__ __launch_bounds__(64) void k_dot_fold(const double* __restrict__ partial, int classes, int entries,
                                                 double* __restrict__ out) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= entries) return;
    out[v] = gram_fold_entry(partial + v, classes, static_cast<size_t>(entries));
}

constexpr int IG_ROW = 65;  // doubles between the rows of the tile: odd

__global__ __launch_bounds__(64) void k_obs_impact_global(ImpactGlobalArgs a, double* __restrict__ out) {
    __shared__ double tile[64 * IG_ROW];
    __shared__ double gs[64];
    const int lane = threadIdx.x, M = a.forecast;
    const int q0 = blockIdx.x * 64, q = q0 + lane;
    const bool valid = q < a.nobs;
    const bool used = valid && a.snap[q] == 0;
    const unsigned long long rows = __ballot(used);
    double c = 0.0;
    for (int k0 = 0; k0 < M; k0 += 64) {
        const int mk = min(64, M - k0);
        __syncthreads();  // the last tile's readers are done
        if (lane < mk) {
            for (int rr = 0; rr < 64; ++rr)
                if (rows >> rr & 1) tile[rr * IG_ROW + lane] = a.pert[static_cast<size_t>(q0 + rr) * M + k0 + lane];
            gs[lane] = a.g[k0 + lane];
        }
        __syncthreads();
        if (used) {
            const double* __restrict__ x = tile + lane * IG_ROW;
#pragma unroll 8
            for (int k = 0; k < mk; ++k) c = c + x[k] * gs[k];
        }
    }
    if (!valid) return;
    double J = 0.0;
    if (used) {
        const double S = c / static_cast<double>(M - 1);
        J = a.dn[q] * S;
    }
    out[a.idx[q]] = J;
}

}  // namespace

size_t ens_dot_partial_doubles(const EnsGeom& g, int forecast, int K) {
    return static_cast<size_t>(gram_classes(forecast, static_cast<long>(g.nx) * g.ny)) * forecast * K;
}

hipError_t ens_launch_dot(const EnsGeom& g, const double* f, int forecast, int truth_member, bool centered, int K,
                          const double* fields, double* partial, double* out, hipStream_t st) {
    const int M = forecast;
    if (M < 1 || M > ESPACE_MAX_MEMBERS || K < 1 || K > DOT_MAX_FIELDS || g.slab > 0x7fffffffL)
        return hipErrorInvalidValue;
    const long cells = static_cast<long>(g.nx) * g.ny;
    const int classes = gram_classes(M, cells);
    const hipError_t attr =
        dynamic_lds_once<k_dot_partial>(sizeof(double) * dot_lds_doubles(ESPACE_MAX_MEMBERS, DOT_MAX_FIELDS));
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(k_dot_partial, dim3(classes), dim3(GRAM_THREADS), sizeof(double) * dot_lds_doubles(M, K), st, f, g.nx, cells,
                       gram_segments(cells), g.pitch, g.slab, M, truth_member, centered ? 1 : 0, K, fields, partial);
    const hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(k_dot_fold, dim3((M * K + 63) / 64), dim3(64), 0, st, partial, classes, M * K, out);
    return hipGetLastError();
}

hipError_t ens_launch_obs_impact_global(const ImpactGlobalArgs& a, double* out, hipStream_t st) {
    if (a.nobs <= 0 || a.forecast < 2 || a.forecast > ESPACE_MAX_MEMBERS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_obs_impact_global, dim3((a.nobs + 63) / 64), dim3(64), 0, st, a, out);
    return hipGetLastError();
}

}  // namespace csim
