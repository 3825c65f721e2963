// ensemble_quantiles.hip — per-cell quantiles and exceedance probabilities over the members of an ensemble
// (csim_ensemble_quantiles*, host side in ensemble_diag.cpp).  Needs only the slab layout of ensemble.hpp, not the sweep core
// (sweep_core.hpp).
//
// For every cell of the reference layout (ny+2) x (nx+2), ghost ring included, with s the members' values in ascending
// order and (lo, hi, g) numpy's "linear" plan of a level (csim_ensemble_quantile_plan, made on the host):
//   a = s[lo]; b = s[hi]; d = b - a;  q = g >= 0.5 ? b - d * (1 - g) : a + d * g;  NaN if any member is NaN
//   p = (members with x > t) / B                                             (IEEE division; a NaN member never counts)
// which is np.quantile(x, q, axis=0) and np.mean(x > t, axis=0) of the stacked members (up to the sign of a zero
// quantile, whose order among +0 / -0 numpy leaves undefined).
//
// The order statistics come from a bitonic network (fmin / fmax compare-exchanges): its control flow is fixed by B
// alone, the same in every lane.  A NaN member makes the network's output meaningless, but also the cell's quantiles
// NaN, so a flag taken before the sort decides; the exceedance counts are taken before the sort too.  The members are
// padded to P = 2^ceil(log2 B) with +inf, which sorts past every real member and leaves s[0 .. B) as it is.
//
// Lane form (B <= 64) and wave form (64 < B <= QUANT_MAX_MEMBERS) as ensemble_cell.hpp describes them; the lane form
// runs one wave per workgroup and picks s[lo] by a wave-uniform index, the wave form writes the sorted column back to
// its tile in place, and one lane per level reads s[lo], s[hi] from there.  The networks' pieces are in
// ensemble_sort.hpp, shared with ensemble_verify.hip.
#include "ensemble_cell.hpp"
#include "ensemble_sort.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

__device__ __forceinline__ double lerp_numpy(double a, double b, double g, bool nan) {
    const double d = b - a;
    const double r = g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
    return nan ? __builtin_nan("") : r;
}

// Form 1: one cell per lane, P (power of two, >= members) values per lane in registers.
template <int P>
__global__ __launch_bounds__(64) void k_quantiles_lane(const double* __restrict__ f, int nx2, int ncells, int pitch,
                                                       long slab, int members, QuantArgs qa, double* __restrict__ out) {
    const int lane = threadIdx.x;
    const int c = blockIdx.x * 64 + lane;
    const bool valid = c < ncells;
    const DenseCell dc = dense_cell(c, nx2, ncells);
    const double* __restrict__ p = cell_ptr(f, dc.i, dc.j, pitch);

    double s[P];
#pragma unroll
    for (int k = 0; k < P; ++k) s[k] = k < members ? p[static_cast<ptrdiff_t>(k) * slab] : __builtin_inf();
    bool nan = false;
#pragma unroll
    for (int k = 0; k < P; ++k) nan |= s[k] != s[k];

    // (the argument arrays are only ever indexed statically: a runtime index would copy them to scratch)
    const double den = static_cast<double>(members);
#pragma unroll
    for (int t = 0; t < QUANT_MAX_LEVELS; ++t) {
        if (t < qa.nt) {  // wave-uniform
            const double thr = qa.thr[t];
            int n = 0;
#pragma unroll
            for (int k = 0; k < P; ++k) n += s[k] > thr;
            if (__builtin_inf() > thr) n -= P - members;  // the +inf pads
            if (valid) out[static_cast<size_t>(qa.nq + t) * ncells + c] = static_cast<double>(n) / den;
        }
    }

    CSIM_SORT_LANE(s, P);  // bitonic network, ascending, static indices throughout

#pragma unroll
    for (int q = 0; q < QUANT_MAX_LEVELS; ++q) {
        if (q < qa.nq) {  // wave-uniform
            const double r = lerp_numpy(pick(s, qa.lo[q]), pick(s, qa.hi[q]), qa.g[q], nan);
            if (valid) out[static_cast<size_t>(q) * ncells + c] = r;
        }
    }
}

// Form 2: one cell per wave, P = 64 E values per wave, tiles of ct cells per four-wave workgroup.
template <int E>
__global__ __launch_bounds__(256) void k_quantiles_wave(const double* __restrict__ f, int nx2, int ncells, int pitch,
                                                        long slab, int members, int ct, int stride, QuantArgs qa,
                                                        double* __restrict__ out) {
    constexpr int P = 64 * E;
    extern __shared__ __attribute__((aligned(16))) double held[];  // [ct][stride], stride odd, >= members
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * ct;

    CSIM_LOAD_TILE(f, nx2, ncells, pitch, slab, members, ct, stride, c0, tid, held);
    __syncthreads();

    // level `lane`'s plan in each lane (static indices only: a runtime index would copy the arguments to scratch)
    int lo = 0, hi = 0;
    double g = 0.0;
#pragma unroll
    for (int q = 0; q < QUANT_MAX_LEVELS; ++q) {
        if (lane == q) {
            lo = qa.lo[q];
            hi = qa.hi[q];
            g = qa.g[q];
        }
    }
    const double den = static_cast<double>(members);
    for (int cl = wave; cl < ct; cl += 4) {  // the same count in every wave: the barrier below is uniform
        const int c = c0 + cl;
        double* col = held + cl * stride;
        double v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int m = e * 64 + lane;
            v[e] = m < members ? col[m] : __builtin_inf();
        }
        bool nan = false;
#pragma unroll
        for (int e = 0; e < E; ++e) nan |= __ballot(v[e] != v[e]) != 0;
#pragma unroll
        for (int t = 0; t < QUANT_MAX_LEVELS; ++t) {
            if (t < qa.nt) {
                const double thr = qa.thr[t];
                int n = 0;
#pragma unroll
                for (int e = 0; e < E; ++e) n += __popcll(__ballot(v[e] > thr));
                if (__builtin_inf() > thr) n -= P - members;
                if (lane == 0 && c < ncells)
                    out[static_cast<size_t>(qa.nq + t) * ncells + c] = static_cast<double>(n) / den;
            }
        }

        for (int k = 2; k <= 64; k <<= 1) cross_stages(v, lane, k, k >> 1);  // merges inside 64 elements
        merges_from<E, 2>(v, lane);

#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int m = e * 64 + lane;
            if (m < members) col[m] = v[e];
        }
        __syncthreads();
        if (lane < qa.nq && c < ncells)  // lane q: level q
            out[static_cast<size_t>(lane) * ncells + c] = lerp_numpy(col[lo], col[hi], g, nan);
    }
}

}  // namespace

hipError_t ens_launch_quantiles(const EnsGeom& g, const double* f, const QuantArgs& qa, double* out, hipStream_t st) {
    const int nx2 = g.nx + 2, ncells = nx2 * (g.ny + 2);
    return for_sort_form(
        g.members,
        [&](auto s) {
            hipLaunchKernelGGL(k_quantiles_lane<decltype(s)::value>, dim3((ncells + 63) / 64), dim3(64), 0, st, f, nx2,
                               ncells, g.pitch, g.slab, g.members, qa, out);
            return hipGetLastError();
        },
        [&](auto s) {
            constexpr int E = decltype(s)::value;
            const SortTile tile = sort_tile(g.members, 0);
            const hipError_t attr = dynamic_lds_once<k_quantiles_wave<E>>(sort_tile(QUANT_MAX_MEMBERS, 0).lds);
            if (attr != hipSuccess) return attr;
            hipLaunchKernelGGL(k_quantiles_wave<E>, dim3((ncells + tile.ct - 1) / tile.ct), dim3(256), tile.lds, st, f,
                               nx2, ncells, g.pitch, g.slab, g.members, tile.ct, tile.stride, qa, out);
            return hipGetLastError();
        });
}

}  // namespace csim
