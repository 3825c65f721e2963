// ensemble_held.hip — observation-space rows that a network holds across run() calls (csim_obs_network_hold and
// csim_ensemble_assimilate_etkf_held of include/csim.h; host side in ensemble_obs.cpp and ensemble_analysis.cpp).  The
// rows are M doubles per plan position, [plan position][member]: the layout of the local analysis's priors
// (k_local_prior of ensemble_local.hip), so 64 consecutive rows are one contiguous run of 64 M doubles.  The Gram
// matrix that reads them is k_obsgram_partial's ROWS form (ensemble_obsgram.hip).  Here:
//   k_obs_hold        one wave per observation of a slot: block b serves plan position list[b] (no list: b), h_k of the
//                     M forecast members through obs_h of obs_wave.hpp into LDS, then one coalesced store of the row.
//                     Neither the mask nor a status byte is looked at: a row is held for every observation.
//   k_held_mv         mv of csim_ensemble_relax over the M values of a row, (mean, variance) by input index into the
//                     arrays that k_obs_screen and k_obs_chunks read (where k_assim_post writes them from the state).
//   k_held_transform  a row as one cell's M members under k_espace_apply<., true>(centered): m, p_k = x_k - m,
//                     m' = m + sum_k p_k wbar[k], x'_r = m' + sum_k p_k W[k M + r], running sums from +0 in member
//                     order; on the device path it obeys the status word that the members' transform obeys.
// The last two work on 64 rows per wave, one row per lane.  The run of 64 M doubles is loaded side by side and put
// into LDS member-major, T[k][lane], rows 65 doubles apart: odd, so that the transposing writes spread over the banks,
// and a lane's walk down its column is free of conflicts (as in k_local_update).  A lane reads and writes its own
// column only, so after the staging no barrier is needed; W and wbar are read with wave-uniform indices, so their loads
// are scalar.  All M values of a row are in LDS before any is written.  Every product and every sum is one rounded
// fp64 operation, no FMA contraction.
#include "obs_wave.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr int HELD_ROWS = 64;    // rows per wave
constexpr int HELD_LD = 65;      // doubles from member k to member k + 1 of the tile
constexpr int HELD_RB = 4;       // outputs r that share one pass over k (CELL_RB of espace_cell.hpp)

inline size_t held_lds(int M) { return sizeof(double) * HELD_LD * static_cast<size_t>(M); }

template <bool LIN>
__global__ __launch_bounds__(64) void k_obs_hold(const double* __restrict__ f, int pitch, long slab, AssimArgs a,
                                                 const int* __restrict__ list, double* __restrict__ rows) {
    extern __shared__ double sh[];  // M values; LIN: linear_lds
    const int M = a.forecast;
    const int q = list ? list[blockIdx.x] : static_cast<int>(blockIdx.x);
    obs_h<LIN>(f, pitch, slab, a, q, sh);
    double* __restrict__ out = rows + static_cast<size_t>(q) * M;
    for (int k = threadIdx.x; k < M; k += 64) out[k] = sh[k];
}

// the nc rows from r0 on into T[k * HELD_LD + c]; element e = c M + k of the run goes through lane e % 64.  Ends with
// a barrier
__device__ __forceinline__ void held_stage(const double* __restrict__ rows, long r0, int nc, int M,
                                           double* __restrict__ T) {
    const double* __restrict__ src = rows + static_cast<size_t>(r0) * M;
    const int lane = threadIdx.x;
    const int n = nc * M, dc = 64 / M, dk = 64 - dc * M;  // what 64 elements further means for (c, k)
    int c = lane / M, k = lane - c * M;
    for (int e = lane; e < n; e += 64) {
        T[k * HELD_LD + c] = src[e];
        c += dc, k += dk;
        if (k >= M) k -= M, ++c;
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void k_held_mv(const double* __restrict__ rows, int nobs, int M,
                                                const int* __restrict__ idx, double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double T[];  // [M][HELD_LD]
    const int lane = threadIdx.x;
    const long r0 = static_cast<long>(blockIdx.x) * HELD_ROWS;
    const int nc = static_cast<int>(min(static_cast<long>(HELD_ROWS), nobs - r0));
    held_stage(rows, r0, nc, M, T);
    if (lane >= nc) return;
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < M; ++k) s = s + T[k * HELD_LD + lane];
    const double m = s / static_cast<double>(M);
    double q = 0.0;
#pragma unroll 8
    for (int k = 0; k < M; ++k) {
        const double d = T[k * HELD_LD + lane] - m;
        q = q + d * d;
    }
    const size_t o = 2 * static_cast<size_t>(idx[r0 + lane]);
    out[o] = m;
    out[o + 1] = q / static_cast<double>(M - 1);
}

__global__ __launch_bounds__(64) void k_held_transform(double* __restrict__ rows, int nobs, int M,
                                                       const double* __restrict__ W, const double* __restrict__ wbar,
                                                       const int* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(16))) double T[];  // [M][HELD_LD]
    // as k_espace_apply: the whole grid returns at once where the weights kernel found nothing to do or a non-finite A
    if (gate && (*gate == ETKF_NONFINITE || *gate == ETKF_SKIP)) return;
    const int lane = threadIdx.x;
    const long r0 = static_cast<long>(blockIdx.x) * HELD_ROWS;
    const int nc = static_cast<int>(min(static_cast<long>(HELD_ROWS), nobs - r0));
    held_stage(rows, r0, nc, M, T);
    if (lane >= nc) return;
    double* __restrict__ x = T + lane;
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < M; ++k) s = s + x[k * HELD_LD];
    const double m = s / static_cast<double>(M);
#pragma unroll 8
    for (int k = 0; k < M; ++k) x[k * HELD_LD] = x[k * HELD_LD] - m;
    double mp = m;
    if (wbar) {
        double d = 0.0;
#pragma unroll 4
        for (int k = 0; k < M; ++k) d = d + x[k * HELD_LD] * wbar[k];
        mp = m + d;
    }
    double* __restrict__ out = rows + static_cast<size_t>(r0 + lane) * M;
    for (int b = 0; b < M; b += HELD_RB) {
        int rr[HELD_RB];
        double acc[HELD_RB];
#pragma unroll
        for (int u = 0; u < HELD_RB; ++u) rr[u] = min(b + u, M - 1), acc[u] = 0.0;
#pragma unroll 4
        for (int k = 0; k < M; ++k) {
            const double pk = x[k * HELD_LD];
#pragma unroll
            for (int u = 0; u < HELD_RB; ++u) acc[u] = acc[u] + pk * W[static_cast<size_t>(k) * M + rr[u]];
        }
#pragma unroll
        for (int u = 0; u < HELD_RB; ++u)
            if (b + u < M) out[b + u] = mp + acc[u];
    }
}

bool held_ok(const double* rows, int nobs, int M) { return rows && nobs >= 1 && M >= 2 && M <= ESPACE_MAX_MEMBERS; }

unsigned held_blocks(int nobs) { return static_cast<unsigned>((nobs + HELD_ROWS - 1) / HELD_ROWS); }

}  // namespace

hipError_t ens_launch_obs_hold(const EnsGeom& g, const double* f, const AssimArgs& a, const int* list, int count,
                               double* rows, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    if (!held_ok(rows, count, a.forecast)) return hipErrorInvalidValue;
    return for_obs_form(a, sizeof(double) * a.forecast, [&](auto lin, size_t lds) {
        hipLaunchKernelGGL(k_obs_hold<decltype(lin)::value>, dim3(count), dim3(64), lds, st, f, g.pitch, g.slab, a, list,
                           rows);
        return hipGetLastError();
    });
}

hipError_t ens_launch_held_mv(const double* rows, int nobs, int M, const int* idx, double* out, hipStream_t st) {
    if (!held_ok(rows, nobs, M) || !idx || !out) return hipErrorInvalidValue;
    const hipError_t attr = dynamic_lds_once<k_held_mv>(held_lds(ESPACE_MAX_MEMBERS));
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(k_held_mv, dim3(held_blocks(nobs)), dim3(64), held_lds(M), st, rows, nobs, M, idx, out);
    return hipGetLastError();
}

hipError_t ens_launch_held_transform(double* rows, int nobs, int M, const double* W, const double* wbar, hipStream_t st,
                                     const int* gate) {
    if (!held_ok(rows, nobs, M) || !W) return hipErrorInvalidValue;
    const hipError_t attr = dynamic_lds_once<k_held_transform>(held_lds(ESPACE_MAX_MEMBERS));
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(k_held_transform, dim3(held_blocks(nobs)), dim3(64), held_lds(M), st, rows, nobs, M, W, wbar,
                       gate);
    return hipGetLastError();
}

}  // namespace csim
