// etkf_weights.hpp — the host mathematics of the ETKF (include/csim.h): the plan of the observation-space Gram sum
// (csim_obs_gram_plan) and the weights (csim_etkf_weights, etkf_weights.cpp).  Plain host code without the HIP headers,
// compiled without FMA contraction; the kernel's launcher (ensemble_obsgram.hip) takes its classes from here.
#pragma once

namespace csim {

constexpr int OBS_GRAM_SEG = 64;           // plan positions per segment
constexpr int OBS_GRAM_MAX_MEMBERS = 256;  // CSIM_ESPACE_MAX_MEMBERS

// classes of the sum for M forecast members (0: M out of range): the caps of csim_ensemble_gram
inline int obs_gram_cap(int M) { return M < 1 ? 0 : M <= 64 ? 1024 : M <= 128 ? 256 : M <= OBS_GRAM_MAX_MEMBERS ? 64 : 0; }
inline long obs_gram_segments(int nobs) { return (static_cast<long>(nobs) + OBS_GRAM_SEG - 1) / OBS_GRAM_SEG; }
inline int obs_gram_classes(int M, int nobs) {
    const long nseg = obs_gram_segments(nobs);
    return static_cast<int>(nseg < obs_gram_cap(M) ? nseg : obs_gram_cap(M));
}

}  // namespace csim
