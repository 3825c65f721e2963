// ensemble_obsgram.hip — the observation-space Gram matrix of csim_ensemble_obs_gram (host side in ensemble_analysis.cpp;
// the definition is the ETKF block of csim.h).  Needs the slab layout of ensemble.hpp; the plan is gram_plan.hpp, and
// the lanes' pairs, the walk over a segment's rows, the class's partial and the fold of an entry are gram_tile.hpp, as
// for k_gram_partial (ensemble_space.hip).  Here: the rows of a segment are 64 consecutive plan positions of a network,
// gathered through its operator and normalised, M + 1 columns wide.
//   k_obsgram_partial  Workgroup (g, y) of 256 lanes serves class g: the segments g, g + Gc, ...  Lane (c, kq) gathers
//                      h_k of observation c for the members k = kq, kq + 4, ... into LDS as [observation][member]: a
//                      point observation is one strided load per member, a linear one the tap loop per (observation,
//                      member), a running sum from +0 in tap order.  An observation that is not used is not read: its
//                      row is +0 and its y and sqrt(r) are kept as 0 and 1, so every z and e of it comes out +0 with
//                      the arithmetic of the others, and +0 leaves a running sum that started from +0 as it is.
//                      LL: lane k of workgroup (g, 0) then adds e_k e_k of the raw rows to its running sum.  64 lanes
//                      form hb, the rows are normalised, z_M goes to column M, and the tile walks the segment's rows.
//                      ROWS (csim_ensemble_obs_gram_held): h_k is read from rows that the network holds, M per plan
//                      position ([plan position][member], ensemble_held.hip), in place of the gather: a segment's 64
//                      rows are one contiguous run of 64 M doubles, which the 256 lanes load side by side and scatter
//                      into the same [observation][member] tile; the flag of every row goes through LDS first, so that
//                      a row that is not used is not read.  Everything after the staging is the text of the others.
//   k_obsgram_fold     entry (a, b), a <= b, folded over the classes and written to A[a][b] and A[b][a]; the row
//                      after the last folds loglik the same way and adds up the counts.
// Every product and every sum is one rounded fp64 operation, no FMA contraction.
#include <algorithm>

#include "gram_tile.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

static_assert(ESPACE_MAX_MEMBERS <= GRAM_THREADS, "one lane per member in the loglik pass");

// dynamic LDS: the rows, then hb, y and sqrt(r) of the segment's observations
inline size_t og_lds(int M) { return sizeof(double) * (static_cast<size_t>(GRAM_SEG) * gram_stride(M + 1) + 3 * GRAM_SEG); }

template <int NB, bool LIN, bool LL, bool ROWS = false>
__global__ __launch_bounds__(GRAM_THREADS) void k_obsgram_partial(
    const double* __restrict__ f, int pitch, long slab, ObsGramArgs a, long nseg, double* __restrict__ partial,
    double* __restrict__ llpart, int* __restrict__ cntpart) {
    extern __shared__ __attribute__((aligned(16))) double held[];  // [64][stride], then hb, y, sr
    const int M = a.forecast, t = a.truth_member, MA = M + 1;
    const int stride = gram_stride(MA);
    double* __restrict__ hbs = held + GRAM_SEG * stride;
    double* __restrict__ ys = hbs + GRAM_SEG;
    double* __restrict__ srs = ys + GRAM_SEG;
    const int tid = threadIdx.x;
    const int mpad = gram_nblk(MA) * GRAM_TB;
    GramTile<NB> tile;
    tile.init(MA);
    double ll = 0.0;
    int cnt = 0;

    const int c = tid & 63, kq = tid >> 6;
    double* __restrict__ row = held + c * stride;
    for (long q = blockIdx.x; q < nseg; q += gridDim.x) {
        const long e0 = q * GRAM_SEG;
        const int nc = static_cast<int>(min(static_cast<long>(GRAM_SEG), a.nobs - e0));
        bool used = false;
        if constexpr (ROWS) {
            // wave 0 decides and publishes the flags (in hbs, which is free until the means); then element e = c M + k
            // of the segment's run goes from lane e % 256 to row c, column k: 256 elements further is (dc, dk) further
            if (kq == 0) {
                const int o = static_cast<int>(e0) + c;
                used = c < nc && (!a.flag || a.flag[o] == a.used);
                hbs[c] = used ? 1.0 : 0.0;
                ys[c] = used ? a.y[o] : 0.0;
                srs[c] = used ? a.sr[o] : 1.0;
            }
            __syncthreads();
            const double* __restrict__ src = a.rows + static_cast<size_t>(e0) * M;
            const int n = nc * M, dc = GRAM_THREADS / M, dk = GRAM_THREADS - dc * M;
            int rc = tid / M, rk = tid - rc * M;
            for (int e = tid; e < n; e += GRAM_THREADS) {
                double v = 0.0;
                if (hbs[rc] != 0.0) v = src[e];
                held[rc * stride + rk] = v;
                rc += dc, rk += dk;
                if (rk >= M) rk -= M, ++rc;
            }
            if (c < nc)
                for (int k = M + kq; k < mpad; k += 4) row[k] = 0.0;
        } else if (c < nc) {
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
        if (tid < nc) hbs[tid] = gram_row_mean(held + tid * stride, M);
        __syncthreads();
        if (c < nc) {
            const double hb = hbs[c], sr = srs[c];
#pragma unroll 8
            for (int k = kq; k < M; k += 4) row[k] = (row[k] - hb) / sr;
            if (kq == 0) row[M] = (ys[c] - hb) / sr;
        }
        __syncthreads();
        tile.walk(held, stride, nc);
        __syncthreads();
    }
    tile.store(partial + static_cast<size_t>(blockIdx.x) * gram_pairs(MA), MA);
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
        if (want_ll && rb < M) llout[rb] = gram_fold_entry(llpart + rb, classes, M);
        if (rb == 0) {
            long long n = 0;
            for (int g = 0; g < classes; ++g) n += cntpart[g];
            *reinterpret_cast<long long*>(llout + M) = n;
        }
        return;
    }
    if (rb < ra || rb >= MA) return;
    const double s = gram_fold_entry(partial + gram_packed(ra, rb, MA), classes, gram_pairs(MA));
    out[static_cast<size_t>(ra) * MA + rb] = s;
    out[static_cast<size_t>(rb) * MA + ra] = s;
}

struct OgPartials {
    size_t ll, cnt, doubles;  // where loglik's and the counts' partials start, and the end, in doubles
};
OgPartials og_partials(int M, int nobs) {
    const size_t classes = static_cast<size_t>(gram_classes(M, nobs));
    OgPartials p{};
    p.ll = classes * gram_pairs(M + 1);
    p.cnt = p.ll + classes * M;
    p.doubles = p.cnt + (classes + 1) / 2;
    return p;
}

template <int NB, bool LIN, bool LL, bool ROWS = false>
hipError_t launch_obsgram(const EnsGeom& g, const double* f, const ObsGramArgs& a, double* partial, double* out,
                          hipStream_t st) {
    const int M = a.forecast, MA = M + 1;
    const int classes = gram_classes(M, a.nobs);
    const OgPartials p = og_partials(M, a.nobs);
    const hipError_t attr = dynamic_lds_once<k_obsgram_partial<NB, LIN, LL, ROWS>>(og_lds(ESPACE_MAX_MEMBERS));
    if (attr != hipSuccess) return attr;
    double* llpart = partial + p.ll;
    int* cntpart = reinterpret_cast<int*>(partial + p.cnt);
    hipLaunchKernelGGL((k_obsgram_partial<NB, LIN, LL, ROWS>), dim3(classes, gram_shares(MA, NB)), dim3(GRAM_THREADS),
                       og_lds(M), st, f, g.pitch, g.slab, a, gram_segments(a.nobs), partial, llpart, cntpart);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(k_obsgram_fold, dim3((MA + 63) / 64, MA + 1), dim3(64), 0, st, partial, llpart, cntpart, classes,
                       M, LL ? 1 : 0, out);
    return hipGetLastError();
}

}  // namespace

size_t ens_obs_gram_partial_doubles(int forecast, int nobs) { return og_partials(forecast, nobs).doubles; }

hipError_t ens_launch_obs_gram(const EnsGeom& g, const double* f, const ObsGramArgs& a, bool want_loglik,
                               double* partial, double* out, int form, hipStream_t st) {
    const int M = a.forecast;
    if (M < 2 || M > ESPACE_MAX_MEMBERS || a.nobs < 1 || form < 0 || form > GRAM_FORMS) return hipErrorInvalidValue;
    return for_gram_form(form, M, [&](auto nb) {
        constexpr int NB = decltype(nb)::value;
        if (a.rows)
            return want_loglik ? launch_obsgram<NB, false, true, true>(g, f, a, partial, out, st)
                               : launch_obsgram<NB, false, false, true>(g, f, a, partial, out, st);
        if (a.tstart)
            return want_loglik ? launch_obsgram<NB, true, true>(g, f, a, partial, out, st)
                               : launch_obsgram<NB, true, false>(g, f, a, partial, out, st);
        return want_loglik ? launch_obsgram<NB, false, true>(g, f, a, partial, out, st)
                           : launch_obsgram<NB, false, false>(g, f, a, partial, out, st);
    });
}

}  // namespace csim
