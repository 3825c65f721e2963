// gram_tile.hpp — the device part of a Gram sum over the geometry of gram_plan.hpp, shared by k_gram_partial
// (ensemble_space.hip), k_dot_partial (ensemble_dot.hip), k_obsgram_partial (ensemble_obsgram.hip) and k_letkf_gram
// (ensemble_letkf.hip).  A segment's rows lie in LDS as [row][column], gram_stride(cols) doubles apart and +0 from
// column cols up to the padded width; the observation kernels stage them their own way.  Here:
//   gram_row_mean    a row's first M columns summed from +0 in column order, over M: the mean of all four kernels.
//   gram_stage_cells a segment of interior cells as rows [cell][member] of p_k, for k_gram_partial and k_dot_partial.
//   gram_block_step  one row onto a block's 16 sums: two 16-byte reads per block side (the lanes of a wave mostly
//                    share the a-side address, which broadcasts, and read neighbouring 32-byte pieces on the b-side),
//                    one rounded product and one rounded sum per pair, no FMA contraction.
//   GramTile<NB>     a lane's NB blocks of 4 x 4 pairs (a, b) and their 16 NB running sums.  walk() adds a segment's
//                    rows in order, a gram_block_step per row and block.  The sums are carried from segment to
//                    segment of a class; which lane owns which pair is geometry: the order of each pair's sum is that
//                    of the rows.  store() writes the class's partial as the packed upper triangle.
//   gram_fold_entry  one entry over the classes: partial 0, then + partial 1, ... in class order.
//   for_gram_form    launch(Step<NB>) with the blocks per lane of a form, form 0: the one chosen from M.
#pragma once

#include "ensemble_cell.hpp"
#include "gram_plan.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

__device__ __forceinline__ double gram_row_mean(const double* __restrict__ x, int M) {
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < M; ++k) s = s + x[k];
    return s / static_cast<double>(M);
}

// The nc <= GRAM_SEG interior cells from e0 on into `held` ([GRAM_SEG][gram_stride(M)], then GRAM_SEG means) as
// [cell][member]: x_k, +0 from member M up to the padded width, less the cell's mean when centered.  All GRAM_THREADS
// lanes call it, lane (c, kq) serves cell c and the members kq, kq + 4, ...  What a caller stages of its own beside
// the rows (the dot's field values) it writes before the call, and the first barrier here publishes that too; after
// the call every lane may read every row.  Rows from nc on keep what the last segment left there.
__device__ __forceinline__ void gram_stage_cells(const double* __restrict__ f, int nx, int pitch, long slab, int M,
                                                 int t, int centered, long e0, int nc, double* __restrict__ held) {
    const int stride = gram_stride(M), mpad = gram_nblk(M) * GRAM_TB;
    double* __restrict__ mean = held + GRAM_SEG * stride;
    const int tid = threadIdx.x, c = tid & 63, kq = tid >> 6;
    double* __restrict__ row = held + c * stride;
    if (c < nc) {
        const Cell cc = cell_of(e0 + c, nx, pitch);
        const double* __restrict__ p = f + static_cast<size_t>(cc.off);
#pragma unroll 8
        for (int k = kq; k < M; k += 4) row[k] = p[static_cast<size_t>(forecast_member(k, t)) * slab];
        for (int k = M + kq; k < mpad; k += 4) row[k] = 0.0;
    }
    __syncthreads();
    if (centered) {
        if (tid < nc) mean[tid] = gram_row_mean(held + tid * stride, M);
        __syncthreads();
        if (c < nc) {
            const double m = mean[c];
#pragma unroll 8
            for (int k = kq; k < M; k += 4) row[k] = row[k] - m;
        }
        __syncthreads();
    }
}

// acc[i GRAM_TB + j] += xa[i] xb[j]: xa, xb 16-byte aligned.  The parameters are not __restrict__ (the two reads
// inside are): with them k_gram_partial<1> takes 102 VGPRs for its 78 and falls from 6 waves per SIMD to 4
__device__ __forceinline__ void gram_block_step(const double* xa, const double* xb,
                                                double (&acc)[GRAM_TB * GRAM_TB]) {
    const double2* __restrict__ pa = reinterpret_cast<const double2*>(xa);
    const double2* __restrict__ pb = reinterpret_cast<const double2*>(xb);
    const double2 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
    const double a[GRAM_TB] = {a0.x, a0.y, a1.x, a1.y};
    const double b[GRAM_TB] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
    for (int i = 0; i < GRAM_TB; ++i)
#pragma unroll
        for (int j = 0; j < GRAM_TB; ++j) acc[i * GRAM_TB + j] = acc[i * GRAM_TB + j] + a[i] * b[j];
}

template <int NB>
struct GramTile {
    int ia[NB], ib[NB];
    bool mine[NB];
    bool wave_on;  // false: this wave only helps staging
    double acc[NB][GRAM_TB * GRAM_TB];

    // workgroup (., share = blockIdx.y), lane threadIdx.x
    __device__ __forceinline__ void init(int cols) {
        const int share = blockIdx.y, lane = threadIdx.x;
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const GramOwned o = gram_owned(share, NB, u, lane, cols);
            ia[u] = o.at.ia, ib[u] = o.at.ib, mine[u] = o.mine;
#pragma unroll
            for (int v = 0; v < GRAM_TB * GRAM_TB; ++v) acc[u][v] = 0.0;
        }
        wave_on = gram_wave_on(share, NB, lane, cols);
    }

    // the rows 0 .. nc - 1 of `held`, in order
    __device__ __forceinline__ void walk(const double* __restrict__ held, int stride, int nc) {
        if (!wave_on) return;
#pragma unroll 2
        for (int cc = 0; cc < nc; ++cc) {
            const double* __restrict__ x = held + cc * stride;
#pragma unroll
            for (int u = 0; u < NB; ++u) gram_block_step(x + GRAM_TB * ia[u], x + GRAM_TB * ib[u], acc[u]);
        }
    }

    __device__ __forceinline__ void store(double* __restrict__ class_partial, int cols) const {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            if (!mine[u]) continue;
#pragma unroll
            for (int i = 0; i < GRAM_TB; ++i)
#pragma unroll
                for (int j = 0; j < GRAM_TB; ++j) {
                    const int a = GRAM_TB * ia[u] + i, b = GRAM_TB * ib[u] + j;
                    if (a <= b && b < cols) class_partial[gram_packed(a, b, cols)] = acc[u][i * GRAM_TB + j];
                }
        }
    }
};

// p: the entry in partial 0; `step` doubles from one class's to the next
__device__ __forceinline__ double gram_fold_entry(const double* __restrict__ p, int classes, size_t step) {
    double s = p[0];
#pragma unroll 16
    for (int g = 1; g < classes; ++g) s = s + p[static_cast<size_t>(g) * step];
    return s;
}

template <class F>
hipError_t for_gram_form(int form, int M, F&& launch) {
    if (form == 0) form = gram_auto_form(M);
    if (form == 1) return launch(Step<gram_form_nb(1)>{});
    if (form == 2) return launch(Step<gram_form_nb(2)>{});
    return launch(Step<gram_form_nb(3)>{});
}

}  // namespace

}  // namespace csim
