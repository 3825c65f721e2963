// ensemble_verify.hip — verification of an ensemble against one truth per cell (csim_ensemble_verify*, host side in
// ensemble_diag.cpp): per-cell CRPS and Brier scores, the rank histogram and the domain scores, from one read of the
// members.  Needs only the slab layout of ensemble.hpp and the sorting networks of ensemble_sort.hpp.
//
// M forecast members x_k and the truth y per cell (csim.h has the whole definition).  Forecast member k is member
// forecast_member(k, t) of the ensemble, t the truth member (or B: none, the truth comes from a dense device field).
// A cell is NaN when y or any x_k is; its CRPS and Brier scores are NaN, and the histogram and the domain scores skip
// it.
//   a = sum |x_k - y|, m = sum x_k / M, v = sum (x_k - m)^2 / (M - 1), lt = #(x_k < y), eq = #(x_k == y)
//   c = sum_{i=1}^{M-1} i (M - i) (s_i - s_{i-1}), s sorted ascending;  CRPS = a / M - c / W, W = M^2 or M (M - 1)
//   Brier_k = (#(x > thr_k) / M - (y > thr_k))^2;  rank = lt + mix(g) mod (eq + 1), g the interior index
// Every sum starts from +0.  The order of the per-cell sums is fixed by M alone:
// Lane form (M <= 64, ensemble_cell.hpp): one cell per lane, the values in registers, four waves per workgroup.  a,
// the sum of x, v, the counts and the Brier scores are taken in member order before the sort (five sums in one member
// loop, so not the header's mean_regs / var_regs), c in sorted order after it (CSIM_SORT_LANE).
// Wave form (64 < M <= 4096): one cell per wave from the LDS tile of ensemble_cell.hpp, the histogram behind the
// tile.  Element k is in lane k % 64; each lane sums its elements in increasing k, and the 64 lane sums l are combined
// as l[i] += l[i ^ h] for h = 32, 16, .., 1 (the same bits in every lane).  c is summed the same way over the sorted
// index i, whose predecessor s_{i-1} is read from the sorted column written back to LDS.
// Each workgroup loops over tiles (at most VERIFY_GRID_MAX workgroups), keeps its rank histogram in LDS and flushes it
// once with one 64-bit atomic per non-empty bin.  Its partial sums of the domain scores are reduced in a fixed order
// (per-lane sums in tile order, the same xor tree across a wave, then waves 0 .. 3) and stored, one record per
// workgroup, for the host to add in workgroup order: the same state always gives the same bits.
#include <algorithm>

#include "ensemble_cell.hpp"
#include "ensemble_sort.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

// l[lane] + l[lane ^ h] for h = 32 .. 1: the whole wave's sum, the same bits in every lane
__device__ __forceinline__ double wave_tree(double x, int lane) {
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) x = x + bpermute(x, (lane ^ h) << 2);
    return x;
}

__device__ __forceinline__ bool interior(int i, int j, int nx, int ny) { return i >= 1 && i <= nx && j >= 1 && j <= ny; }

__device__ __forceinline__ int rank_of(int lt, int eq, int i, int j, int nx) {
    const unsigned long long g = static_cast<unsigned long long>(j - 1) * nx + (i - 1);
    return lt + static_cast<int>(verify_mix(g) % static_cast<unsigned long long>(eq + 1));
}

__device__ __forceinline__ double brier(int n, double den, double y, double thr) {
    const double p = static_cast<double>(n) / den;
    const double d = p - (y > thr ? 1.0 : 0.0);
    return d * d;
}

// the end of both forms: the LDS histogram flushed, wsum[w][q] (wave w's sum q) and the counts stored as this
// workgroup's record
__device__ __forceinline__ void finish_block(const VerifyArgs& va, const VerifyOut& o, const unsigned* hist,
                                             double (*wsum)[VERIFY_SUMS], const unsigned* cnt) {
    const int tid = threadIdx.x;
    for (int b = tid; b <= va.forecast; b += 256)
        if (hist[b]) atomicAdd(o.hist + b, static_cast<unsigned long long>(hist[b]));
    if (tid < 3 + va.nt) {
        double x = wsum[0][tid];
        x = x + wsum[1][tid];
        x = x + wsum[2][tid];
        x = x + wsum[3][tid];
        o.sums[static_cast<size_t>(blockIdx.x) * VERIFY_SUMS + tid] = x;
    }
    if (tid < 2) o.counts[2 * static_cast<size_t>(blockIdx.x) + tid] = cnt[tid];
}

// Form 1: one cell per lane, P (power of two, >= M) values per lane in registers, 256 cells per tile.
template <int P>
__global__ __launch_bounds__(256) void k_verify_lane(const double* __restrict__ f, int nx, int ny, int pitch, long slab,
                                                     VerifyArgs va, VerifyOut o) {
    __shared__ unsigned hist[P + 1];
    __shared__ double bsum[VERIFY_MAX_THRESHOLDS][256];  // each thread's Brier sums (registers would cost 32 VGPRs)
    __shared__ double wsum[4][VERIFY_SUMS];
    __shared__ unsigned cnt[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = va.forecast, t = va.truth_member;
    const int nx2 = nx + 2, ncells = nx2 * (ny + 2);
    for (int b = tid; b <= M; b += 256) hist[b] = 0;
    if (tid < 2) cnt[tid] = 0;
#pragma unroll
    for (int q = 0; q < VERIFY_MAX_THRESHOLDS; ++q)
        if (q < va.nt) bsum[q][tid] = 0.0;
    __syncthreads();

    const double den = static_cast<double>(M), vden = static_cast<double>(M - 1);
    const double wden = static_cast<double>(va.fair ? M * (M - 1) : M * M);
    double s_crps = 0.0, s_sq = 0.0, s_var = 0.0;
    unsigned n_ok = 0, n_nan = 0;
    for (int c0 = blockIdx.x * 256; c0 < ncells; c0 += gridDim.x * 256) {
        const int c = c0 + tid;
        const bool valid = c < ncells;
        const DenseCell dc = dense_cell(c, nx2, ncells);
        const int cc = dc.c, i = dc.i, j = dc.j;
        const double* __restrict__ p = cell_ptr(f, i, j, pitch);

        double s[P];
#pragma unroll
        for (int k = 0; k < P; ++k)
            s[k] = k < M ? p[static_cast<ptrdiff_t>(forecast_member(k, t)) * slab] : __builtin_inf();
        const double y = va.truth ? va.truth[cc] : p[static_cast<ptrdiff_t>(t) * slab];
        bool nan = y != y;
#pragma unroll
        for (int k = 0; k < P; ++k) nan |= s[k] != s[k];

        // member order, before the sort
        double a = 0.0, sum = 0.0;
        int lt = 0, eq = 0;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            if (k < M) {
                a = a + fabs(s[k] - y);
                sum = sum + s[k];
                lt += s[k] < y;
                eq += s[k] == y;
            }
        }
        const double m = sum / den;
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            if (k < M) {
                const double d = s[k] - m;
                v = v + d * d;
            }
        }
        v = v / vden;
        const bool counted = valid && interior(i, j, nx, ny) && !nan;
#pragma unroll
        for (int q = 0; q < VERIFY_MAX_THRESHOLDS; ++q) {
            if (q < va.nt) {  // wave-uniform
                const double thr = va.thr[q];
                int n = 0;
#pragma unroll
                for (int k = 0; k < P; ++k) n += k < M && s[k] > thr;
                const double bs = brier(n, den, y, thr);
                if (valid) o.brier[static_cast<size_t>(q) * ncells + c] = nan ? __builtin_nan("") : bs;
                if (counted) bsum[q][tid] = bsum[q][tid] + bs;
            }
        }
        const double dm = m - y;
        const double sq = dm * dm;
        const int rank = counted ? rank_of(lt, eq, i, j, nx) : 0;

        CSIM_SORT_LANE(s, P);
        double g = 0.0;
#pragma unroll
        for (int k = 1; k < P; ++k)
            if (k < M) g = g + static_cast<double>(k * (M - k)) * (s[k] - s[k - 1]);
        const double crps = a / den - g / wden;
        if (valid) o.crps[c] = nan ? __builtin_nan("") : crps;
        if (counted) {
            s_crps = s_crps + crps;
            s_sq = s_sq + sq;
            s_var = s_var + v;
            ++n_ok;
            atomicAdd(hist + rank, 1u);
        } else if (valid && interior(i, j, nx, ny)) {
            ++n_nan;
        }
    }

#pragma unroll
    for (int q = 0; q < VERIFY_SUMS; ++q) {
        if (q < 3 + va.nt) {
            const double x = q == 0 ? s_crps : q == 1 ? s_sq : q == 2 ? s_var : bsum[q < 3 ? 0 : q - 3][tid];
            const double w = wave_tree(x, lane);
            if (lane == 0) wsum[wave][q] = w;
        }
    }
    atomicAdd(cnt, n_ok);
    atomicAdd(cnt + 1, n_nan);
    __syncthreads();
    finish_block(va, o, hist, wsum, cnt);
}

// Form 2: one cell per wave, 64 E values per wave (M of them real, +inf pads), tiles of ct cells x all B members per four-wave workgroup.
template <int E>
__global__ __launch_bounds__(256) void k_verify_wave(const double* __restrict__ f, int nx, int ny, int pitch, long slab,
                                                     int members, int ct, int stride, VerifyArgs va, VerifyOut o) {
    extern __shared__ __attribute__((aligned(16))) double held[];  // [ct][stride] (stride odd, >= B), then M + 1 bins
    __shared__ double wsum[4][VERIFY_SUMS];  // wave w's running sums (lane 0 adds), then its totals
    __shared__ unsigned cnt[2];
    unsigned* hist = reinterpret_cast<unsigned*>(held + ct * stride);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = va.forecast, t = va.truth_member;
    const int nx2 = nx + 2, ncells = nx2 * (ny + 2);
    for (int b = tid; b <= M; b += 256) hist[b] = 0;
    if (tid < 4 * VERIFY_SUMS) wsum[tid / VERIFY_SUMS][tid % VERIFY_SUMS] = 0.0;
    if (tid < 2) cnt[tid] = 0;

    const double den = static_cast<double>(M), vden = static_cast<double>(M - 1);
    const double wden = static_cast<double>(va.fair ? M * (M - 1) : M * M);
    const int tiles = (ncells + ct - 1) / ct;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int c0 = tile * ct;
        __syncthreads();  // the previous tile's reads are done (and the zeroing above)
        CSIM_LOAD_TILE(f, nx2, ncells, pitch, slab, members, ct, stride, c0, tid, held);
        __syncthreads();

        for (int cl = wave; cl < ct; cl += 4) {  // the same count in every wave: the barrier below is uniform
            const int c = c0 + cl;
            const DenseCell dc = dense_cell(c, nx2, ncells);
            const int cc = dc.c, i = dc.i, j = dc.j;
            double* col = held + cl * stride;
            const double y = va.truth ? va.truth[cc] : col[t];
            double v[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int k = e * 64 + lane;
                v[e] = k < M ? col[forecast_member(k, t)] : __builtin_inf();
            }
            bool nan = y != y;
#pragma unroll
            for (int e = 0; e < E; ++e) nan |= __ballot(v[e] != v[e]) != 0;

            double a = 0.0, sum = 0.0;
            int lt = 0, eq = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const bool in = e * 64 + lane < M;
                if (in) {
                    a = a + fabs(v[e] - y);
                    sum = sum + v[e];
                }
                lt += __popcll(__ballot(in && v[e] < y));
                eq += __popcll(__ballot(in && v[e] == y));
            }
            a = wave_tree(a, lane);
            const double mean = wave_tree(sum, lane) / den;
            double var = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (e * 64 + lane < M) {
                    const double d = v[e] - mean;
                    var = var + d * d;
                }
            }
            var = wave_tree(var, lane) / vden;
            const bool counted = c < ncells && interior(i, j, nx, ny) && !nan;
#pragma unroll
            for (int q = 0; q < VERIFY_MAX_THRESHOLDS; ++q) {
                if (q < va.nt) {
                    const double thr = va.thr[q];
                    int n = 0;
#pragma unroll
                    for (int e = 0; e < E; ++e) n += __popcll(__ballot(e * 64 + lane < M && v[e] > thr));
                    const double bs = brier(n, den, y, thr);
                    if (lane == 0) {
                        if (c < ncells) o.brier[static_cast<size_t>(q) * ncells + c] = nan ? __builtin_nan("") : bs;
                        if (counted) wsum[wave][3 + q] = wsum[wave][3 + q] + bs;
                    }
                }
            }

            for (int k = 2; k <= 64; k <<= 1) cross_stages(v, lane, k, k >> 1);  // merges inside 64 elements
            merges_from<E, 2>(v, lane);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int k = e * 64 + lane;
                if (k < M) col[k] = v[e];
            }
            __syncthreads();
            double g = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int k = e * 64 + lane;
                if (k >= 1 && k < M) g = g + static_cast<double>(k * (M - k)) * (v[e] - col[k - 1]);
            }
            g = wave_tree(g, lane);
            const double crps = a / den - g / wden;
            if (lane == 0) {
                if (c < ncells) o.crps[c] = nan ? __builtin_nan("") : crps;
                if (counted) {
                    const double dm = mean - y;
                    wsum[wave][0] = wsum[wave][0] + crps;
                    wsum[wave][1] = wsum[wave][1] + dm * dm;
                    wsum[wave][2] = wsum[wave][2] + var;
                    atomicAdd(cnt, 1u);
                    atomicAdd(hist + rank_of(lt, eq, i, j, nx), 1u);
                } else if (c < ncells && interior(i, j, nx, ny)) {
                    atomicAdd(cnt + 1, 1u);
                }
            }
        }
    }
    __syncthreads();
    finish_block(va, o, hist, wsum, cnt);
}

// the wave form's tile of all B members with the M + 1 bins of the histogram behind it
SortTile wave_tile(int members, int forecast) { return sort_tile(members, sizeof(unsigned) * (forecast + 1)); }

}  // namespace

int ens_verify_blocks(const EnsGeom& g, int forecast) {
    const int ncells = (g.nx + 2) * (g.ny + 2);
    const int cells = forecast <= 64 ? 256 : wave_tile(g.members, forecast).ct;
    return std::min((ncells + cells - 1) / cells, VERIFY_GRID_MAX);
}

hipError_t ens_launch_verify(const EnsGeom& g, const double* f, const VerifyArgs& va, const VerifyOut& o,
                             hipStream_t st) {
    const int M = va.forecast;
    if (M < 1 || va.nt < 0 || va.nt > VERIFY_MAX_THRESHOLDS) return hipErrorInvalidValue;
    return for_sort_form(
        M,
        [&](auto s) {
            hipLaunchKernelGGL(k_verify_lane<decltype(s)::value>, dim3(ens_verify_blocks(g, M)), dim3(256), 0, st, f,
                               g.nx, g.ny, g.pitch, g.slab, va, o);
            return hipGetLastError();
        },
        [&](auto s) {
            constexpr int E = decltype(s)::value;
            const SortTile tile = wave_tile(g.members, M);
            // the largest tile: 4 cells of B = VERIFY_MAX_MEMBERS + 1 members (a truth member and 4096 others)
            const hipError_t attr =
                dynamic_lds_once<k_verify_wave<E>>(wave_tile(VERIFY_MAX_MEMBERS + 1, VERIFY_MAX_MEMBERS).lds);
            if (attr != hipSuccess) return attr;
            hipLaunchKernelGGL(k_verify_wave<E>, dim3(ens_verify_blocks(g, M)), dim3(256), tile.lds, st, f, g.nx, g.ny,
                               g.pitch, g.slab, g.members, tile.ct, tile.stride, va, o);
            return hipGetLastError();
        });
}

}  // namespace csim
