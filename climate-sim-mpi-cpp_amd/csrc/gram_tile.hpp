// gram_tile.hpp — the device part of a Gram sum over the geometry of gram_plan.hpp, shared by k_gram_partial
// (ensemble_space.hip) and k_obsgram_partial (ensemble_obsgram.hip).  A kernel stages a segment's rows in LDS as
// [row][column], gram_stride(cols) doubles apart and +0 from column cols up to the padded width, its own way; here:
//   GramTile<NB>     a lane's NB blocks of 4 x 4 pairs (a, b) and their 16 NB running sums.  walk() adds a segment's
//                    rows in order: two 16-byte reads per block side (the lanes of a wave mostly share the a-side
//                    address, which broadcasts, and read neighbouring 32-byte pieces on the b-side), one rounded
//                    product and one rounded sum per pair, no FMA contraction.  The sums are carried from segment to
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
            for (int u = 0; u < NB; ++u) {
                const double2* __restrict__ pa = reinterpret_cast<const double2*>(x + GRAM_TB * ia[u]);
                const double2* __restrict__ pb = reinterpret_cast<const double2*>(x + GRAM_TB * ib[u]);
                const double2 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
                const double a[GRAM_TB] = {a0.x, a0.y, a1.x, a1.y};
                const double b[GRAM_TB] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                for (int i = 0; i < GRAM_TB; ++i)
#pragma unroll
                    for (int j = 0; j < GRAM_TB; ++j) acc[u][i * GRAM_TB + j] = acc[u][i * GRAM_TB + j] + a[i] * b[j];
            }
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
