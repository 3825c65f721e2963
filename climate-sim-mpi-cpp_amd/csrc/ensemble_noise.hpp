// ensemble_noise.hpp — the random numbers of csim_ensemble_perturb, exactly as include/csim.h defines them, for host
// (csim_philox4x32, csim_normal_from_bits) and device (ensemble_perturb.hip) alike: Philox4x32-10 and a normal deviate
// from 64 bits through Wichura's AS241 (PPND16) with the library's own logarithm.  Integer arithmetic, + - * / and sqrt
// only, no FMA contraction, so both sides and a numpy restatement give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

namespace csim {

constexpr int PERTURB_MAX_RADIUS = 32;  // CSIM_PERTURB_MAX_RADIUS

__host__ __device__ inline unsigned noise_mulhi(unsigned a, unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return static_cast<unsigned>((static_cast<unsigned long long>(a) * b) >> 32);
#endif
}

// Philox4x32-10 (Salmon et al. 2011): c the counter, k the key, the result replaces c
__host__ __device__ inline void philox4x32(unsigned c[4], unsigned k0, unsigned k1) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = noise_mulhi(M0, c[0]), l0 = M0 * c[0];
        const unsigned h1 = noise_mulhi(M1, c[2]), l1 = M1 * c[2];
        c[0] = h1 ^ c[1] ^ k0, c[1] = l1, c[2] = h0 ^ c[3] ^ k1, c[3] = l0;
        k0 += W0, k1 += W1;
    }
}

// sum_{n=0..7} co[n] x^n, from the highest coefficient
__host__ __device__ inline double noise_horner(const double (&co)[8], double x) {
    double r = co[7];
#pragma unroll
    for (int n = 6; n >= 0; --n) r = r * x + co[n];
    return r;
}

// ln t for a normal t > 0: frexp, the fold at sqrt(1/2), and 2 atanh(s) as an odd series to s^23
__host__ __device__ inline double noise_log(double t) {
    union {
        double d;
        unsigned long long u;
    } v;
    v.d = t;
    int e = static_cast<int>((v.u >> 52) & 0x7ffu) - 1022;
    v.u = (v.u & 0x800fffffffffffffull) | 0x3fe0000000000000ull;  // frexp's mantissa, in [0.5, 1)
    double m = v.d;
    if (m < 0x1.6a09e667f3bcdp-1) m = m * 2.0, e = e - 1;
    const double s = (m - 1.0) / (m + 1.0);
    const double w = s * s;
    double p = 1.0 / 23.0;
    p = p * w + 1.0 / 21.0;
    p = p * w + 1.0 / 19.0;
    p = p * w + 1.0 / 17.0;
    p = p * w + 1.0 / 15.0;
    p = p * w + 1.0 / 13.0;
    p = p * w + 1.0 / 11.0;
    p = p * w + 1.0 / 9.0;
    p = p * w + 1.0 / 7.0;
    p = p * w + 1.0 / 5.0;
    p = p * w + 1.0 / 3.0;
    p = p * w + 1.0;
    return static_cast<double>(e) * 0x1.62e42fefa39efp-1 + 2.0 * (s * p);
}

// the standard normal quantile of u = (k + 0.5) 2^-52, k the upper 52 bits
__host__ __device__ inline double normal_from_bits(unsigned long long bits) {
    constexpr double A[8] = {3.3871328727963666080e0,  1.3314166789178437745e2, 1.9715909503065514427e3,
                             1.3731693765509461125e4,  4.5921953931549871457e4, 6.7265770927008700853e4,
                             3.3430575583588128105e4,  2.5090809287301226727e3};
    constexpr double B[8] = {1.0,                      4.2313330701600911252e1, 6.8718700749205790830e2,
                             5.3941960214247511077e3,  2.1213794301586595867e4, 3.9307895800092710610e4,
                             2.8729085735721942674e4,  5.2264952788528545610e3};
    constexpr double Cc[8] = {1.42343711074968357734e0,  4.63033784615654529590e0,  5.76949722146069140550e0,
                              3.64784832476320460504e0,  1.27045825245236838258e0,  2.41780725177450611770e-1,
                              2.27238449892691845833e-2, 7.74545014278341407640e-4};
    constexpr double Dd[8] = {1.0,                       2.05319162663775882187e0,  1.67638483018380384940e0,
                              6.89767334985100004550e-1, 1.48103976427480074590e-1, 1.51986665636164571966e-2,
                              5.47593808499534494600e-4, 1.05075007164441684324e-9};
    constexpr double E[8] = {6.65790464350110377720e0,  5.46378491116411436990e0,  1.78482653991729133580e0,
                             2.96560571828504891230e-1, 2.65321895265761230930e-2, 1.24266094738807843860e-3,
                             2.71155556874348757815e-5, 2.01033439929228813265e-7};
    constexpr double F[8] = {1.0,                       5.99832206555887937690e-1, 1.36929880922735805310e-1,
                             1.48753612908506148525e-2, 7.86869131145613259100e-4, 1.84631831751005468180e-5,
                             1.42151175831644588870e-7, 2.04426310338993978564e-15};
    const double u = (static_cast<double>(bits >> 12) + 0.5) * 0x1p-52;
    const double q = u - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return q * noise_horner(A, r) / noise_horner(B, r);
    }
    const double t = q < 0.0 ? u : 1.0 - u;
    const double r = sqrt(-noise_log(t));
    double z;
    if (r <= 5.0) {
        const double x = r - 1.6;
        z = noise_horner(Cc, x) / noise_horner(Dd, x);
    } else {
        const double x = r - 5.0;
        z = noise_horner(E, x) / noise_horner(F, x);
    }
    return q < 0.0 ? -z : z;
}

}  // namespace csim
