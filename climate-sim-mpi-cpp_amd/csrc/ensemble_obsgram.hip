// ensemble_obsgram.hip — the observation-space Gram matrix of csim_ensemble_obs_gram (host side in ensemble_obs.cpp;
// the definition is the ETKF block of csim.h).  Needs the slab layout of ensemble.hpp and the plan of etkf_weights.hpp.
//
// The structure of k_gram_partial (ensemble_space.hip) with another staging stage: the rows of a segment are 64
// consecutive plan positions of a network, gathered through its operator, instead of 64 contiguous cells.
//   k_obsgram_partial  Workgroup (g, y) of 256 lanes serves class g: the segments g, g + Gc, ...  Lane (c, kq) gathers
//                      h_k of observation c for the members k = kq, kq + 4, ... into LDS as [observation][member]: a
//                      point observation is one strided load per member, a linear one the tap loop per (observation,
//                      member), a running sum from +0 in tap order.  An observation that is not used is not read: its
//                      row is +0 and its y and sqrt(r) are kept as 0 and 1, so every z and e of it comes out +0 with
//                      the arithmetic of the others, and +0 leaves a running sum that started from +0 as it is.
//                      LL: lane k of workgroup (g, 0) then adds e_k e_k of the raw rows to its running sum.  64 lanes
//                      form hb, the rows are normalised, z_M goes to column M, and every lane walks the segment's rows
//                      in order for its NB blocks of 4 x 4 pairs of the upper triangle of the (M + 1) x (M + 1)
//                      matrix, carrying the 16 NB running sums on to the class's next segment.  Which lane owns which
//                      pair is geometry: the order of each pair's sum is that of the plan positions.
//   k_obsgram_fold     entry (a, b), a <= b: partial 0, then + partial 1, ... + partial Gc - 1, written to A[a][b] and
//                      A[b][a]; the row after the last folds loglik the same way and adds up the counts.
// Every product and every sum is one rounded fp64 operation, no FMA contraction.
#include <algorithm>

#include "ensemble_cell.hpp"
#include "etkf_weights.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr int OG_THREADS = 256;
constexpr int OG_TB = 4;  // pairs per block side
static_assert(OBS_GRAM_MAX_MEMBERS <= OG_THREADS, "one lane per member in the loglik pass");
static_assert(OBS_GRAM_MAX_MEMBERS == ESPACE_MAX_MEMBERS, "the two limits are one");

// row stride for MA = M + 1 columns: even, so a lane's four columns are one or two 16-byte reads
__host__ __device__ inline int og_stride(int MA) { return (MA + OG_TB - 1) / OG_TB * OG_TB + 2; }
// dynamic LDS: the rows, then hb, y and sqrt(r) of the segment's observations
inline size_t og_lds(int M) { return sizeof(double) * (static_cast<size_t>(OBS_GRAM_SEG) * og_stride(M + 1) + 3 * OBS_GRAM_SEG); }

template <int NB, bool LIN, bool LL>
__global__ __launch_bounds__(OG_THREADS) void k_obsgram_partial(const double* __restrict__ f, int pitch, long slab,
                                                                ObsGramArgs a, long nseg, double* __restrict__ partial,
                                                                double* __restrict__ llpart, int* __restrict__ cntpart) {
    extern __shared__ __attribute__((aligned(16))) double held[];  // [64][stride], then hb, y, sr
    const int M = a.forecast, t = a.truth_member, MA = M + 1;
    const int stride = og_stride(MA);
    double* __restrict__ hbs = held + OBS_GRAM_SEG * stride;
    double* __restrict__ ys = hbs + OBS_GRAM_SEG;
    double* __restrict__ srs = ys + OBS_GRAM_SEG;
    const int tid = threadIdx.x;
    const int nblk = (MA + OG_TB - 1) / OG_TB;
    const int nblocks = nblk * (nblk + 1) / 2;
    const int mpad = nblk * OG_TB;

    // this lane's blocks (ia <= ib), row by row of the block triangle; past the end: the last one, computed and dropped
    int ia[NB], ib[NB];
    bool mine[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int bidx = (blockIdx.y * NB + u) * OG_THREADS + tid;
        mine[u] = bidx < nblocks;
        int r = min(bidx, nblocks - 1), b = 0;
        while (r >= nblk - b) r -= nblk - b, ++b;
        ia[u] = b, ib[u] = b + r;
    }
    // a wave none of whose lanes owns a block only helps staging
    const bool wave_on = blockIdx.y * NB * OG_THREADS + (tid & ~63) < nblocks;

    double acc[NB][OG_TB * OG_TB];
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
        for (int v = 0; v < OG_TB * OG_TB; ++v) acc[u][v] = 0.0;
    double ll = 0.0;
    int cnt = 0;

    const int c = tid & 63, kq = tid >> 6;
    double* __restrict__ row = held + c * stride;
    for (long q = blockIdx.x; q < nseg; q += gridDim.x) {
        const long e0 = q * OBS_GRAM_SEG;
        const int nc = static_cast<int>(min(static_cast<long>(OBS_GRAM_SEG), a.nobs - e0));
        bool used = false;
        if (c < nc) {
            const int o = static_cast<int>(e0) + c;
            used = !a.flag || a.flag[o] == a.used;
            if (used) {
                const double* __restrict__ p = cell_ptr(f, a.i[o], a.j[o], pitch);
                if constexpr (LIN) {
                    const int s0 = a.tstart[o], s1 = a.tstart[o + 1];
                    for (int k = kq; k < M; k += 4) {
                        const double* __restrict__ pk = p + static_cast<size_t>(forecast_member(k, t)) * slab;
                        double h = 0.0;
                        for (int s = s0; s < s1; ++s) h = h + a.tw[s] * pk[a.toff[s]];
                        row[k] = h;
                    }
                } else {
#pragma unroll 8
                    for (int k = kq; k < M; k += 4) row[k] = p[static_cast<size_t>(forecast_member(k, t)) * slab];
                }
                for (int k = M + kq; k < mpad; k += 4) row[k] = 0.0;
            } else {
                for (int k = kq; k < mpad; k += 4) row[k] = 0.0;
            }
            if (kq == 0) {
                ys[c] = used ? a.y[o] : 0.0;
                srs[c] = used ? a.sr[o] : 1.0;
            }
        }
        if (kq == 0) cnt += __popcll(__ballot(used));  // wave 0 holds one lane per observation
        __syncthreads();
        if constexpr (LL) {
            if (blockIdx.y == 0 && tid < M) {
                for (int cc = 0; cc < nc; ++cc) {
                    const double e = (ys[cc] - held[cc * stride + tid]) / srs[cc];
                    ll = ll + e * e;
                }
            }
        }
        if (tid < nc) {
            const double* __restrict__ x = held + tid * stride;
            double s = 0.0;
#pragma unroll 8
            for (int k = 0; k < M; ++k) s = s + x[k];
            hbs[tid] = s / static_cast<double>(M);
        }
        __syncthreads();
        if (c < nc) {
            const double hb = hbs[c], sr = srs[c];
#pragma unroll 8
            for (int k = kq; k < M; k += 4) row[k] = (row[k] - hb) / sr;
            if (kq == 0) row[M] = (ys[c] - hb) / sr;
        }
        __syncthreads();
        if (wave_on) {
#pragma unroll 2
            for (int cc = 0; cc < nc; ++cc) {
                const double* __restrict__ x = held + cc * stride;
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const double2* __restrict__ pa = reinterpret_cast<const double2*>(x + OG_TB * ia[u]);
                    const double2* __restrict__ pb = reinterpret_cast<const double2*>(x + OG_TB * ib[u]);
                    const double2 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
                    const double va[OG_TB] = {a0.x, a0.y, a1.x, a1.y};
                    const double vb[OG_TB] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                    for (int i = 0; i < OG_TB; ++i)
#pragma unroll
                        for (int j = 0; j < OG_TB; ++j)
                            acc[u][i * OG_TB + j] = acc[u][i * OG_TB + j] + va[i] * vb[j];
                }
            }
        }
        __syncthreads();
    }

    const size_t pairs = static_cast<size_t>(MA) * (MA + 1) / 2;
    double* __restrict__ mine_out = partial + static_cast<size_t>(blockIdx.x) * pairs;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if (!mine[u]) continue;
#pragma unroll
        for (int i = 0; i < OG_TB; ++i)
#pragma unroll
            for (int j = 0; j < OG_TB; ++j) {
                const int ra = OG_TB * ia[u] + i, rb = OG_TB * ib[u] + j;
                if (ra <= rb && rb < MA)
                    mine_out[static_cast<size_t>(ra) * MA - static_cast<size_t>(ra) * (ra - 1) / 2 + (rb - ra)] =
                        acc[u][i * OG_TB + j];
            }
    }
    if (blockIdx.y == 0) {
        if constexpr (LL) {
            if (tid < M) llpart[static_cast<size_t>(blockIdx.x) * M + tid] = ll;
        }
        if (tid == 0) cntpart[blockIdx.x] = cnt;
    }
}

// grid (ceil(MA / 64), MA + 1): row a = blockIdx.y < MA, column b; row MA: loglik entry b and the count
__global__ __launch_bounds__(64) void k_obsgram_fold(const double* __restrict__ partial,
                                                     const double* __restrict__ llpart,
                                                     const int* __restrict__ cntpart, int classes, int M, int want_ll,
                                                     double* __restrict__ out) {
    const int MA = M + 1;
    const int ra = blockIdx.y, rb = blockIdx.x * 64 + threadIdx.x;
    double* __restrict__ llout = out + static_cast<size_t>(MA) * MA;
    if (ra == MA) {
        if (want_ll && rb < M) {
            double s = llpart[rb];
            for (int g = 1; g < classes; ++g) s = s + llpart[static_cast<size_t>(g) * M + rb];
            llout[rb] = s;
        }
        if (rb == 0) {
            long long n = 0;
            for (int g = 0; g < classes; ++g) n += cntpart[g];
            *reinterpret_cast<long long*>(llout + M) = n;
        }
        return;
    }
    if (rb < ra || rb >= MA) return;
    const size_t pairs = static_cast<size_t>(MA) * (MA + 1) / 2;
    const double* __restrict__ p =
        partial + (static_cast<size_t>(ra) * MA - static_cast<size_t>(ra) * (ra - 1) / 2 + (rb - ra));
    double s = p[0];
#pragma unroll 16
    for (int g = 1; g < classes; ++g) s = s + p[static_cast<size_t>(g) * pairs];
    out[static_cast<size_t>(ra) * MA + rb] = s;
    out[static_cast<size_t>(rb) * MA + ra] = s;
}

struct OgPartials {
    size_t ll, cnt, doubles;  // where loglik's and the counts' partials start, and the end, in doubles
};
OgPartials og_partials(int M, int nobs) {
    const size_t classes = static_cast<size_t>(obs_gram_classes(M, nobs));
    const size_t pairs = static_cast<size_t>(M + 1) * (M + 2) / 2;
    OgPartials p{};
    p.ll = classes * pairs;
    p.cnt = p.ll + classes * M;
    p.doubles = p.cnt + (classes + 1) / 2;
    return p;
}

template <int NB, bool LIN, bool LL>
hipError_t launch_obsgram(const EnsGeom& g, const double* f, const ObsGramArgs& a, double* partial, double* out,
                          hipStream_t st) {
    const int M = a.forecast, MA = M + 1;
    const long nseg = obs_gram_segments(a.nobs);
    const int classes = obs_gram_classes(M, a.nobs);
    const int nblk = (MA + OG_TB - 1) / OG_TB;
    const int nblocks = nblk * (nblk + 1) / 2;
    const int shares = (nblocks + NB * OG_THREADS - 1) / (NB * OG_THREADS);
    const OgPartials p = og_partials(M, a.nobs);
    const hipError_t attr = dynamic_lds_once<k_obsgram_partial<NB, LIN, LL>>(og_lds(OBS_GRAM_MAX_MEMBERS));
    if (attr != hipSuccess) return attr;
    double* llpart = partial + p.ll;
    int* cntpart = reinterpret_cast<int*>(partial + p.cnt);
    hipLaunchKernelGGL((k_obsgram_partial<NB, LIN, LL>), dim3(classes, shares), dim3(OG_THREADS), og_lds(M), st, f,
                       g.pitch, g.slab, a, nseg, partial, llpart, cntpart);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(k_obsgram_fold, dim3((MA + 63) / 64, MA + 1), dim3(64), 0, st, partial, llpart, cntpart, classes,
                       M, LL ? 1 : 0, out);
    return hipGetLastError();
}

template <int NB>
hipError_t launch_obsgram_nb(const EnsGeom& g, const double* f, const ObsGramArgs& a, bool ll, double* partial,
                             double* out, hipStream_t st) {
    if (a.tstart)
        return ll ? launch_obsgram<NB, true, true>(g, f, a, partial, out, st)
                  : launch_obsgram<NB, true, false>(g, f, a, partial, out, st);
    return ll ? launch_obsgram<NB, false, true>(g, f, a, partial, out, st)
              : launch_obsgram<NB, false, false>(g, f, a, partial, out, st);
}

}  // namespace

size_t ens_obs_gram_partial_doubles(int forecast, int nobs) { return og_partials(forecast, nobs).doubles; }

hipError_t ens_launch_obs_gram(const EnsGeom& g, const double* f, const ObsGramArgs& a, bool want_loglik,
                               double* partial, double* out, int form, hipStream_t st) {
    const int M = a.forecast;
    if (M < 2 || M > OBS_GRAM_MAX_MEMBERS || a.nobs < 1 || form < 0 || form > OBS_GRAM_FORMS) return hipErrorInvalidValue;
    if (form == 0) form = M <= 64 ? 1 : M <= 128 ? 2 : 3;  // the choice of csim_ensemble_gram
    if (form == 1) return launch_obsgram_nb<1>(g, f, a, want_loglik, partial, out, st);
    if (form == 2) return launch_obsgram_nb<2>(g, f, a, want_loglik, partial, out, st);
    return launch_obsgram_nb<4>(g, f, a, want_loglik, partial, out, st);
}

}  // namespace csim
