// sweepO_inst.hip — one depth of the overlapped-strip sweep: sweepO.hpp plus the explicit instantiation of
// sweepO_T<CSIM_INST_T>.  Built six times (csrc/Makefile, -DCSIM_INST_T=2..7) in parallel with kernels.hip — and, with
// -DCSIM_INST_WIDE, once more for each depth that has wide strips (sweepO_wide_T<6>, <7>: the same kernels with the
// bodies of four columns per lane, register-allocated for those).
#ifndef CSIM_INST_T
#error "sweepO_inst.hip is compiled with -DCSIM_INST_T=<2..7>, once per depth of the fused sweep"
#endif
#include "sweepO.hpp"

namespace csim {

#ifdef CSIM_INST_WIDE
template hipError_t sweepO_wide_T<CSIM_INST_T>(const double* in, double* out, int pitch, const Phys& p, const SweepCfg& cfg,
                                               const Bc2& bc, const FinLines& fin, const SweepPlan& plan, hipStream_t st,
                                               const FrameSync& fs, const unsigned* lease);
#else
template hipError_t sweepO_T<CSIM_INST_T>(const double* in, double* out, int pitch, const Phys& p, const SweepCfg& cfg,
                                          const Bc2& bc, const FinLines& fin, const SweepPlan& plan, hipStream_t st,
                                          const FrameSync& fs, const unsigned* lease);
#endif

}  // namespace csim
