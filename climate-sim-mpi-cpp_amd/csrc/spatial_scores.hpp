// spatial_scores.hpp — the host-only part of the neighbourhood and probability verification, without a device or the HIP
// headers (spatial_scores.cpp): the overflow bound and, behind include/csim.h, csim_verify_spatial_limit and
// csim_verify_spatial_finish.  tools/spatial_host_check.cpp compiles it with plain g++ under AddressSanitizer.
#pragma once
#include "obs_taps.hpp"

namespace csim {

// CSIM_OK, or CSIM_ERR_UNSUPPORTED: more than CSIM_SPATIAL_MAX_MEMBERS forecast members, or M^2 w^4 nx ny > 2^62 with
// w = 2 half_max + 1.  The arguments are in range (M, nx, ny >= 1, 0 <= half_max <= CSIM_SPATIAL_MAX_HALF)
int spatial_limit(int M, long nx, long ny, int half_max);

}  // namespace csim
