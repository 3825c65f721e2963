// ensemble_obs.hip — the kernels of the observation network (csim_obs_network_* in include/csim.h, host side in
// ensemble_obs.cpp).  Needs only the slab layout of ensemble.hpp and the random numbers of ensemble_noise.hpp.
//
//   k_obs_observe  one lane per observation (plan position q): the gather of x_s(i, j) from the source member, and
//                  with noise one Philox call on the counter (input index, 0, 0xFFFFFFFF, draw) and the normal
//                  quantile of its first 64 bits; stores y and xt in plan order.  The deviate depends on the input
//                  index alone, so neither the plan nor the launch geometry shows in the result.  Linear
//                  observations (a.tstart): xt = h of the source member, sum_s w_s x(anchor + tap s) in tap order
//                  from +0; the taps of a footprint are neighbours, so a lane's loads stay in a few cache lines.
//                  LIST (csim_obs_network_observe_slot): the lanes serve the plan positions of a list, the observations
//                  of one time slot; every other observation keeps y and xt.
//   k_obs_chunks   one lane per chunk of OBS_CHUNK consecutive input indices: T_c of the eleven sums of a
//                  csim_obs_cycle, each a running sum from +0 in input order.
//   k_obs_cycle    one wave: lane f folds T_c of sum f in chunk order from +0 into the log's record.
//   k_obs_screen   one lane per plan position: the status byte of csim_ensemble_assimilate_screened, plan order, from
//                  the mask and, with the background check, y, r and the (hb, vb) that k_assim_post has just written.
// SCR instantiations of k_obs_chunks / k_obs_cycle: an observation whose status is not 0 adds nothing (a running sum
// that started from +0 is never -0, so adding +0 leaves its bits) and y of it is not read; three counts per chunk are
// folded in chunk order into n and the screen record.  The SCR = false ones compute what the kernels computed before.
// The background and posterior diagnostics that k_obs_chunks reads are written by the analysis's own k_assim_post
// (ens_launch_assim_post), before and after the analysis.  Every product is rounded, no FMA contraction.
#include "ensemble.hpp"
#include "ensemble_noise.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

template <bool LIN, bool LIST = false>
__global__ __launch_bounds__(256) void k_obs_observe(const double* __restrict__ f, int pitch, long slab, ObsArgs a,
                                                     int member, unsigned seed_lo, unsigned seed_hi, unsigned draw,
                                                     int noise, const int* __restrict__ list = nullptr, int count = 0) {
    int q = blockIdx.x * 256 + threadIdx.x;
    if constexpr (LIST) {
        if (q >= count) return;
        q = list[q];
    }
    if (q >= a.nobs) return;
    const double* p = f + static_cast<ptrdiff_t>(member) * slab + static_cast<ptrdiff_t>(a.j[q]) * pitch + (LPAD - 1) +
                      a.i[q];
    double xt;
    if constexpr (LIN) {
        xt = 0.0;
        for (int s = a.tstart[q]; s < a.tstart[q + 1]; ++s) xt = xt + a.tw[s] * p[a.toff[s]];
    } else {
        xt = *p;
    }
    double y = xt;
    if (noise) {
        unsigned c[4] = {static_cast<unsigned>(a.idx[q]), 0u, 0xFFFFFFFFu, draw};
        philox4x32(c, seed_lo, seed_hi);
        const double z = normal_from_bits(static_cast<unsigned long long>(c[0]) |
                                          (static_cast<unsigned long long>(c[1]) << 32));
        y = xt + a.sr[q] * z;
    }
    a.y[q] = y;
    a.xt[q] = xt;
}

template <bool SCR>
__global__ __launch_bounds__(64) void k_obs_chunks(ObsArgs a, int nchunks, int has_truth,
                                                   const unsigned char* __restrict__ status, int* __restrict__ cnt) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nchunks) return;
    double s[OBS_SUMS];
#pragma unroll
    for (int k = 0; k < OBS_SUMS; ++k) s[k] = 0.0;
    int n[OBS_SCREEN_FIELDS] = {0, 0, 0};
    const int o1 = min(a.nobs, (c + 1) * OBS_CHUNK);
    for (int o = c * OBS_CHUNK; o < o1; ++o) {
        const int q = a.pos[o];
        if constexpr (SCR) {
            const int st = status[q];
            n[0] += st == 0, n[1] += st == 1, n[2] += st >= 2;
            if (st) continue;
        }
        const double y = a.y[q];
        const double hb = a.bg[2 * static_cast<size_t>(o)], vb = a.bg[2 * static_cast<size_t>(o) + 1];
        const double ha = a.post[2 * static_cast<size_t>(o)], va = a.post[2 * static_cast<size_t>(o) + 1];
        const double ob = y - hb, oa = y - ha, ab = ha - hb;
        s[0] = s[0] + ob;
        s[1] = s[1] + ob * ob;
        s[2] = s[2] + oa;
        s[3] = s[3] + oa * oa;
        s[4] = s[4] + oa * ob;
        s[5] = s[5] + ab * ob;
        s[6] = s[6] + vb;
        s[7] = s[7] + va;
        s[8] = s[8] + a.r[q];
        if (has_truth) {
            const double xt = a.xt[q];
            const double eb = hb - xt, ea = ha - xt;
            s[9] = s[9] + eb * eb;
            s[10] = s[10] + ea * ea;
        }
    }
#pragma unroll
    for (int k = 0; k < OBS_SUMS; ++k) a.part[static_cast<size_t>(c) * OBS_SUMS + k] = s[k];
    if constexpr (SCR) {
#pragma unroll
        for (int k = 0; k < OBS_SCREEN_FIELDS; ++k) cnt[static_cast<size_t>(c) * OBS_SCREEN_FIELDS + k] = n[k];
    }
}

template <bool SCR>
__global__ __launch_bounds__(64) void k_obs_cycle(const double* __restrict__ part, int nchunks, int nobs, int has_truth,
                                                  double* __restrict__ slot, const int* __restrict__ cnt,
                                                  double* __restrict__ sslot) {
    const int k = threadIdx.x;
    if constexpr (SCR) {
        if (k < OBS_SCREEN_FIELDS) {
            int n = 0;
            for (int c = 0; c < nchunks; ++c) n += cnt[static_cast<size_t>(c) * OBS_SCREEN_FIELDS + k];
            sslot[k] = static_cast<double>(n);
            if (k == 0) slot[0] = static_cast<double>(n);
        }
        if (k == 0) slot[1] = has_truth ? 1.0 : 0.0;
    } else if (k == 0) {
        slot[0] = static_cast<double>(nobs);
        slot[1] = has_truth ? 1.0 : 0.0;
    }
    if (k >= OBS_SUMS) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s = s + part[static_cast<size_t>(c) * OBS_SUMS + k];
    slot[2 + k] = s;
}

// status: INACTIVE where the mask says so (y is not looked at), else REJECTED iff the check is made and
// !(t t <= k2 (vb + r)), t = y - hb: a NaN rejects, equality keeps; every product rounded
__global__ __launch_bounds__(256) void k_obs_screen(ObsArgs a, ObsScreen s) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.nobs) return;
    unsigned char st = 0;
    if (s.mask && !s.mask[q]) {
        st = 1;
    } else if (s.check) {
        const size_t o = 2 * static_cast<size_t>(a.idx[q]);
        const double t = a.y[q] - s.bg[o];
        const double lhs = t * t;
        const double rhs = s.k2 * (s.bg[o + 1] + a.r[q]);
        if (!(lhs <= rhs)) st = 2;
    }
    s.status[q] = st;
}

__global__ __launch_bounds__(256) void k_obs_screen_log_fill(double* __restrict__ slog, int cycles, int nobs) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cycles) return;
    slog[static_cast<size_t>(c) * OBS_SCREEN_FIELDS] = static_cast<double>(nobs);
    slog[static_cast<size_t>(c) * OBS_SCREEN_FIELDS + 1] = 0.0;
    slog[static_cast<size_t>(c) * OBS_SCREEN_FIELDS + 2] = 0.0;
}

}  // namespace

hipError_t ens_launch_obs_observe(const EnsGeom& g, const double* f, const ObsArgs& a, int member, unsigned seed_lo,
                                  unsigned seed_hi, unsigned draw, bool noise, hipStream_t st) {
    if (a.nobs <= 0 || member < 0 || member >= g.members) return hipErrorInvalidValue;
    if (a.tstart)
        hipLaunchKernelGGL(k_obs_observe<true>, dim3((a.nobs + 255) / 256), dim3(256), 0, st, f, g.pitch, g.slab, a,
                           member, seed_lo, seed_hi, draw, noise ? 1 : 0);
    else
        hipLaunchKernelGGL(k_obs_observe<false>, dim3((a.nobs + 255) / 256), dim3(256), 0, st, f, g.pitch, g.slab, a,
                           member, seed_lo, seed_hi, draw, noise ? 1 : 0);
    return hipGetLastError();
}

hipError_t ens_launch_obs_observe_list(const EnsGeom& g, const double* f, const ObsArgs& a, const int* list, int count,
                                       int member, unsigned seed_lo, unsigned seed_hi, unsigned draw, bool noise,
                                       hipStream_t st) {
    if (count <= 0) return hipSuccess;
    if (a.nobs <= 0 || count > a.nobs || !list || member < 0 || member >= g.members) return hipErrorInvalidValue;
    if (a.tstart)
        hipLaunchKernelGGL((k_obs_observe<true, true>), dim3((count + 255) / 256), dim3(256), 0, st, f, g.pitch, g.slab,
                           a, member, seed_lo, seed_hi, draw, noise ? 1 : 0, list, count);
    else
        hipLaunchKernelGGL((k_obs_observe<false, true>), dim3((count + 255) / 256), dim3(256), 0, st, f, g.pitch, g.slab,
                           a, member, seed_lo, seed_hi, draw, noise ? 1 : 0, list, count);
    return hipGetLastError();
}

hipError_t ens_launch_obs_cycle(const ObsArgs& a, bool has_truth, double* slot, hipStream_t st) {
    if (a.nobs <= 0) return hipErrorInvalidValue;
    const int nchunks = (a.nobs + OBS_CHUNK - 1) / OBS_CHUNK;
    hipLaunchKernelGGL(k_obs_chunks<false>, dim3((nchunks + 63) / 64), dim3(64), 0, st, a, nchunks, has_truth ? 1 : 0,
                       nullptr, nullptr);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_obs_cycle<false>, dim3(1), dim3(64), 0, st, a.part, nchunks, a.nobs, has_truth ? 1 : 0, slot,
                       nullptr, nullptr);
    return hipGetLastError();
}

hipError_t ens_launch_obs_screen(const ObsArgs& a, const ObsScreen& s, hipStream_t st) {
    if (a.nobs <= 0 || !s.status || (s.check && !s.bg)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_obs_screen, dim3((a.nobs + 255) / 256), dim3(256), 0, st, a, s);
    return hipGetLastError();
}

hipError_t ens_launch_obs_cycle_screened(const ObsArgs& a, const ObsScreen& s, bool has_truth, double* slot,
                                         double* sslot, hipStream_t st) {
    if (a.nobs <= 0 || !s.status || !s.cnt || !sslot) return hipErrorInvalidValue;
    const int nchunks = (a.nobs + OBS_CHUNK - 1) / OBS_CHUNK;
    hipLaunchKernelGGL(k_obs_chunks<true>, dim3((nchunks + 63) / 64), dim3(64), 0, st, a, nchunks, has_truth ? 1 : 0,
                       s.status, s.cnt);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_obs_cycle<true>, dim3(1), dim3(64), 0, st, a.part, nchunks, a.nobs, has_truth ? 1 : 0, slot,
                       s.cnt, sslot);
    return hipGetLastError();
}

hipError_t ens_launch_obs_screen_log_fill(double* slog, int cycles, int nobs, hipStream_t st) {
    if (cycles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_obs_screen_log_fill, dim3((cycles + 255) / 256), dim3(256), 0, st, slog, cycles, nobs);
    return hipGetLastError();
}

}  // namespace csim
