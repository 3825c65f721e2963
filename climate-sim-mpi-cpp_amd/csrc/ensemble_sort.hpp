// ensemble_sort.hpp — the bitonic sorting networks shared by the per-cell order statistics of an ensemble
// (ensemble_quantiles.hip, ensemble_verify.hip).  Device code only; every piece is force-inlined into its kernel.
//
// The networks sort ascending with fmin / fmax compare-exchanges; their control flow is fixed by the padded size
// alone, the same in every lane.  A NaN makes the output meaningless, so a caller flags NaN before it sorts.
// Form 1: P (power of two) values per lane in registers, static register indices throughout (CSIM_SORT_LANE).
// Form 2: one sequence of P = 64 E values per wave, element e*64 + lane in v[e] of that lane: strides >= 64 inside
// each lane with static indices, strides below 64 across lanes through ds_bpermute (cross_stages for the merges
// inside 64 elements, then merges_from<E, 2>).
// Wrapping either network in a function of its own changes how the kernels around it are scheduled, so the kernels
// spell out these calls themselves.
#pragma once

#include <hip/hip_runtime.h>

namespace csim {

namespace {

__device__ __forceinline__ void cmpx(double& a, double& b) {  // a <- min, b <- max
    const double lo = fmin(a, b), hi = fmax(a, b);
    a = lo;
    b = hi;
}

// s[k] for a wave-uniform k (kernel argument) without dynamic register indexing.  Masks rather than selects: a chain
// of `k == i ? s[i] : r` is folded into a load through a selected pointer, which sends s to scratch.
template <int P>
__device__ __forceinline__ double pick(const double (&s)[P], int k) {
    unsigned long long r = 0;
#pragma unroll
    for (int i = 0; i < P; ++i) r |= __builtin_bit_cast(unsigned long long, s[i]) & (0ull - (k == i));
    return __builtin_bit_cast(double, r);
}

// lane src/4's x (two ds_bpermute_b32; __shfl_xor's double form goes through memory)
__device__ __forceinline__ double bpermute(double x, int src) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = __builtin_amdgcn_ds_bpermute(src, static_cast<int>(b));
    const unsigned hi = __builtin_amdgcn_ds_bpermute(src, static_cast<int>(b >> 32));
    return __builtin_bit_cast(double, (static_cast<unsigned long long>(hi) << 32) | lo);
}

// Form 1's network on an array s of P (power of two) doubles: bitonic, ascending, static indices throughout.  A macro,
// not a function: the network is unrolled inside its kernel (a function would be unrolled on its own first).
#define CSIM_SORT_LANE(s, P)                                                                                          \
    _Pragma("unroll") for (int k_ = 2; k_ <= (P); k_ <<= 1) {                                                        \
        _Pragma("unroll") for (int h_ = k_ >> 1; h_ > 0; h_ >>= 1) {                                                 \
            _Pragma("unroll") for (int e_ = 0; e_ < (P); ++e_) {                                                     \
                const int o_ = e_ ^ h_;                                                                             \
                if (o_ > e_) {                                                                                      \
                    if ((e_ & k_) == 0) cmpx((s)[e_], (s)[o_]);                                                     \
                    else cmpx((s)[o_], (s)[e_]);                                                                    \
                }                                                                                                   \
            }                                                                                                       \
        }                                                                                                           \
    }

// Form 2's network, element e*64 + lane in v[e] of that lane.  Strides below 64 go across lanes; the merge size k
// and the stride are runtime values there (the register index is static either way).
template <int E>
__device__ __forceinline__ void cross_stages(double (&v)[E], int lane, int k, int h0) {
    for (int h = h0; h > 0; h >>= 1) {
        const bool lower = (lane & h) == 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double y = bpermute(v[e], (lane ^ h) << 2);
            const bool up = (((e << 6) | lane) & k) == 0;
            v[e] = lower == up ? fmin(v[e], y) : fmax(v[e], y);
        }
    }
}

// merges of K * 64 .. P elements: strides K/2 .. 1 (x 64) inside each lane with static indices and directions,
// then strides 32 .. 1 across lanes.  Runtime strides inside a lane would need a choice among register pairs, which
// the compiler turns into pointers and scratch.
template <int E, int K>
__device__ __forceinline__ void merges_from(double (&v)[E], int lane) {
    if constexpr (K <= E) {
#pragma unroll
        for (int H = K / 2; H > 0; H >>= 1) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int o = e ^ H;
                if (o > e) {
                    if ((e & K) == 0) cmpx(v[e], v[o]);
                    else cmpx(v[o], v[e]);
                }
            }
        }
        cross_stages(v, lane, K * 64, 32);
        merges_from<E, 2 * K>(v, lane);
    }
}

}  // namespace

}  // namespace csim
