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
// Form 1 (B <= 64): one cell per lane, as the statistics kernel: a one-wave workgroup owns 64 consecutive cells, each
// member's 64 values one coalesced 512-B load, P values per lane in registers, a fully unrolled network with static
// register indices (instantiated per P = 1 .. 64).  s[lo] is picked by a wave-uniform index.
// Form 2 (64 < B <= QUANT_MAX_MEMBERS): one cell per wave.  Four waves load a tile of CT consecutive cells x B members
// into LDS, CT cells per member load (coalesced), cell-major with an odd row stride so that both the tile's stores and a
// wave's reads down one cell's members are free of bank conflicts.  A wave then holds its cell as E = P/64 values per
// lane (element e*64 + lane), runs the strides >= 64 inside each lane and the others across lanes (ds_bpermute), writes
// the sorted column back in place, and one lane per level reads s[lo], s[hi] from there (instantiated per E = 2 .. 64).
// The networks' pieces are in ensemble_sort.hpp, shared with ensemble_verify.hip.
#include "ensemble.hpp"
#include "ensemble_sort.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr int QUANT_LDS_BUDGET = 64 * 1024;  // form 2 tile target: two workgroups (eight waves) per CU
constexpr int QUANT_TILE_MAX = 16;           // form 2 cells per tile, at most

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
    const int cc = valid ? c : ncells - 1;  // lanes past the end load a real cell and store nothing
    const int j = cc / nx2, i = cc - j * nx2;
    const double* __restrict__ p = f + static_cast<ptrdiff_t>(j) * pitch + (LPAD - 1) + i;

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

    {  // the tile: thread tid loads cell tid % ct of members tid / ct, + 256 / ct, ...; ct consecutive cells per member
        const int cl = tid & (ct - 1);
        const int c = min(c0 + cl, ncells - 1);
        const int j = c / nx2, i = c - j * nx2;
        const double* __restrict__ p = f + static_cast<ptrdiff_t>(j) * pitch + (LPAD - 1) + i;
        const int step = 256 / ct;
        double* row = held + cl * stride;
        int m = tid / ct;
        for (; m + 7 * step < members; m += 8 * step) {
            double x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = p[static_cast<ptrdiff_t>(m + u * step) * slab];
#pragma unroll
            for (int u = 0; u < 8; ++u) row[m + u * step] = x[u];
        }
        for (; m < members; m += step) row[m] = p[static_cast<ptrdiff_t>(m) * slab];
    }
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

template <int P>
hipError_t launch_lane(const EnsGeom& g, const double* f, const QuantArgs& qa, double* out, hipStream_t st) {
    const int nx2 = g.nx + 2, ncells = nx2 * (g.ny + 2);
    hipLaunchKernelGGL(k_quantiles_lane<P>, dim3((ncells + 63) / 64), dim3(64), 0, st, f, nx2, ncells, g.pitch, g.slab,
                       g.members, qa, out);
    return hipGetLastError();
}

template <int E>
hipError_t launch_wave(const EnsGeom& g, const double* f, const QuantArgs& qa, double* out, hipStream_t st) {
    const int nx2 = g.nx + 2, ncells = nx2 * (g.ny + 2);
    const int stride = g.members | 1;
    int ct = QUANT_TILE_MAX;
    while (ct > 4 && static_cast<size_t>(ct) * stride * sizeof(double) > QUANT_LDS_BUDGET) ct >>= 1;
    const size_t lds = static_cast<size_t>(ct) * stride * sizeof(double);
    static const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(k_quantiles_wave<E>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(4 * sizeof(double) * (QUANT_MAX_MEMBERS | 1)));
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(k_quantiles_wave<E>, dim3((ncells + ct - 1) / ct), dim3(256), lds, st, f, nx2, ncells, g.pitch,
                       g.slab, g.members, ct, stride, qa, out);
    return hipGetLastError();
}

}  // namespace

hipError_t ens_launch_quantiles(const EnsGeom& g, const double* f, const QuantArgs& qa, double* out, hipStream_t st) {
    const int B = g.members;
    if (B <= 1) return launch_lane<1>(g, f, qa, out, st);
    if (B <= 2) return launch_lane<2>(g, f, qa, out, st);
    if (B <= 4) return launch_lane<4>(g, f, qa, out, st);
    if (B <= 8) return launch_lane<8>(g, f, qa, out, st);
    if (B <= 16) return launch_lane<16>(g, f, qa, out, st);
    if (B <= 32) return launch_lane<32>(g, f, qa, out, st);
    if (B <= 64) return launch_lane<64>(g, f, qa, out, st);
    if (B <= 128) return launch_wave<2>(g, f, qa, out, st);
    if (B <= 256) return launch_wave<4>(g, f, qa, out, st);
    if (B <= 512) return launch_wave<8>(g, f, qa, out, st);
    if (B <= 1024) return launch_wave<16>(g, f, qa, out, st);
    if (B <= 2048) return launch_wave<32>(g, f, qa, out, st);
    if (B <= QUANT_MAX_MEMBERS) return launch_wave<64>(g, f, qa, out, st);
    return hipErrorInvalidValue;  // the host refuses these first
}

}  // namespace csim
