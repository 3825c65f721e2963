// ensemble_spatial.hip — neighbourhood and probability verification of an ensemble (csim_ensemble_verify_spatial*, host
// side in ensemble_spatial.cpp; csim.h has the whole definition).  Everything here is an integer: how many forecast
// members exceed a threshold in a cell (n_q), whether the truth does (o_q), and sums of those over square windows.
// Integer addition is exact and commutative, so no result depends on the launch geometry, on the order in which
// workgroups finish or on how the members of a cell are split.  Needs only the slab layout of ensemble.hpp.
//
// Two passes, because a window of up to 65 x 65 cells would make a fused kernel read the members' halo several times
// over, while the count planes are 2 bytes per cell and threshold against 8 M bytes of members:
//
// k_spatial_counts   one lane per interior cell e = (j - 1) nx + (i - 1), consecutive lanes on consecutive i, so every
//   member row is one coalesced 512-byte read per wavefront.  The lane streams over its forecast members, eight loads
//   in flight, and keeps the nt counters in registers; the thresholds are kernel arguments (scalar registers).  No
//   sorting, so there is no lane / wave form by M.  Many members on few cells (1024 x 64^2 is 64 wavefronts of cells)
//   leave the chip idle: then blockIdx.y splits the members of a cell into parts, each part adds its counts with
//   32-bit atomics into a zeroed scratch plane, and k_spatial_merge turns the sums into the count planes and the
//   flags.  The host decides the split from cells and M (ens_spatial_split).
//
// k_spatial_scores   grid (tiles, nt).  A workgroup takes tiles of 32 x 32 centres.  Per tile it loads the count plane
//   and the truth bits of the centres and of a halo of the call's own largest half-width H (zero outside the interior;
//   NaN cells already hold zeros) into LDS and turns both into summed-area tables in place, side 32 + 2 H + 1 (row 0
//   and column 0 are zero): row prefix sums, one row per lane, then column prefix sums, one column per lane; the odd
//   side keeps both free of bank conflicts.  32-bit entries for n (at most M (32 + 2 H)^2 < 2^26), 16-bit for o (at
//   most 96^2).  Every scale then costs four reads per table and centre, whatever its width.  A lane adds F F, O O and
//   F O of its centres in 64-bit registers; after the last tile they are summed across the wave, then across the
//   workgroup through LDS, and the workgroup issues one 64-bit atomic per (q, s, sum).  The same workgroup
//   histograms (n_q, o_q) of its centres into 2 (M + 1) LDS bins and flushes the non-empty ones with 64-bit atomics;
//   threshold 0's workgroups also add the cell and NaN-cell counts.
//   LDS per workgroup: 208 + 6 (32 + 2 H + 1)^2 + 8 (M + 1) bytes: 56.7 KiB of tables at H = 32, 6.7 KiB at H = 0;
//   at or below 64 KiB (two workgroups per CU) for every M at H <= 20 and for M <= 1105 at H = 32.
#include <algorithm>

#include "ensemble_cell.hpp"

namespace csim {

namespace {

constexpr int T = SPATIAL_TILE;

// Pass 1.  SPLIT: the members k0 .. k1 - 1 of this blockIdx.y only, added into o.acc
template <bool SPLIT>
__global__ __launch_bounds__(256) void k_spatial_counts(const double* __restrict__ f, int nx, int ny, int pitch,
                                                        long slab, SpatialArgs a, SpatialOut o) {
    const int M = a.forecast, t = a.truth_member;
    const int cells = nx * ny;
    const int part = (M + a.split - 1) / a.split;
    const int k0 = SPLIT ? static_cast<int>(blockIdx.y) * part : 0;
    const int k1 = SPLIT ? min(M, k0 + part) : M;
    for (int e0 = blockIdx.x * 256; e0 < cells; e0 += gridDim.x * 256) {
        const int e = e0 + threadIdx.x;
        const bool valid = e < cells;
        const int ec = min(e, cells - 1);  // lanes past the end load the last cell and store nothing
        const int j0 = ec / nx, i0 = ec - j0 * nx;
        const double* __restrict__ p = cell_ptr(f, i0 + 1, j0 + 1, pitch);

        unsigned cnt[VERIFY_MAX_THRESHOLDS] = {};
        bool nan = false;
        int k = k0;
        for (; k + 8 <= k1; k += 8) {
            double x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = p[static_cast<ptrdiff_t>(forecast_member(k + u, t)) * slab];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                nan |= x[u] != x[u];
#pragma unroll
                for (int q = 0; q < VERIFY_MAX_THRESHOLDS; ++q)
                    if (q < a.nt) cnt[q] += x[u] > a.thr[q];  // wave-uniform
            }
        }
        for (; k < k1; ++k) {
            const double x = p[static_cast<ptrdiff_t>(forecast_member(k, t)) * slab];
            nan |= x != x;
#pragma unroll
            for (int q = 0; q < VERIFY_MAX_THRESHOLDS; ++q)
                if (q < a.nt) cnt[q] += x > a.thr[q];
        }

        if (SPLIT) {
            if (valid) {
#pragma unroll
                for (int q = 0; q < VERIFY_MAX_THRESHOLDS; ++q)
                    if (q < a.nt && cnt[q]) atomicAdd(o.acc + static_cast<size_t>(q) * cells + e, cnt[q]);
                if (nan) atomicOr(o.acc + static_cast<size_t>(a.nt) * cells + e, 1u);
            }
        } else {
            const double y = a.truth ? a.truth[static_cast<size_t>(j0 + 1) * (nx + 2) + (i0 + 1)]
                                     : p[static_cast<ptrdiff_t>(t) * slab];
            nan |= y != y;
            unsigned fl = nan ? 0x80000000u : 0u;
#pragma unroll
            for (int q = 0; q < VERIFY_MAX_THRESHOLDS; ++q) {
                if (q < a.nt) {
                    if (!nan && y > a.thr[q]) fl |= 1u << q;
                    if (valid) o.counts[static_cast<size_t>(q) * cells + e] = static_cast<unsigned short>(nan ? 0u : cnt[q]);
                }
            }
            if (valid) o.flags[e] = fl;
        }
    }
}

// the end of a split pass 1: the summed parts and the truth -> count planes and flags
__global__ __launch_bounds__(256) void k_spatial_merge(const double* __restrict__ f, int nx, int ny, int pitch, long slab,
                                                       SpatialArgs a, SpatialOut o) {
    const int cells = nx * ny;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < cells; e += gridDim.x * 256) {
        const int j0 = e / nx, i0 = e - j0 * nx;
        const double y = a.truth ? a.truth[static_cast<size_t>(j0 + 1) * (nx + 2) + (i0 + 1)]
                                 : cell_ptr(f, i0 + 1, j0 + 1, pitch)[static_cast<ptrdiff_t>(a.truth_member) * slab];
        const bool nan = y != y || o.acc[static_cast<size_t>(a.nt) * cells + e] != 0u;
        unsigned fl = nan ? 0x80000000u : 0u;
        for (int q = 0; q < a.nt; ++q) {
            if (!nan && y > a.thr[q]) fl |= 1u << q;
            o.counts[static_cast<size_t>(q) * cells + e] =
                static_cast<unsigned short>(nan ? 0u : o.acc[static_cast<size_t>(q) * cells + e]);
        }
        o.flags[e] = fl;
    }
}

__host__ __device__ constexpr size_t round16(size_t b) { return (b + 15) & ~static_cast<size_t>(15); }
// the dynamic LDS of pass 2: the workgroup's 24 sums and 2 counts, the two tables, the histogram
constexpr size_t SCORES_HEAD = 8 * 3 * SPATIAL_MAX_SCALES + 16;

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) x += __shfl_xor(x, h);
    return x;
}

// Pass 2
__global__ __launch_bounds__(256) void k_spatial_scores(int nx, int ny, SpatialArgs a, SpatialOut o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int M = a.forecast, H = a.hmax, q = blockIdx.y;
    const int W = T + 2 * H + 1, WW = W * W;
    unsigned long long* red = reinterpret_cast<unsigned long long*>(smem);           // [s][3]
    unsigned* cnt = reinterpret_cast<unsigned*>(smem + 8 * 3 * SPATIAL_MAX_SCALES);  // non-NaN, NaN centres
    unsigned* sn = reinterpret_cast<unsigned*>(smem + SCORES_HEAD);                  // [W][W]
    unsigned short* so = reinterpret_cast<unsigned short*>(smem + SCORES_HEAD + round16(4 * static_cast<size_t>(WW)));
    unsigned* hist = reinterpret_cast<unsigned*>(smem + SCORES_HEAD + round16(4 * static_cast<size_t>(WW)) +
                                                 round16(2 * static_cast<size_t>(WW)));  // [M + 1][2]
    if (tid < 3 * SPATIAL_MAX_SCALES) red[tid] = 0ull;
    if (tid < 2) cnt[tid] = 0u;
    for (int b = tid; b < 2 * (M + 1); b += 256) hist[b] = 0u;

    const int tilesx = (nx + T - 1) / T, tilesy = (ny + T - 1) / T, tiles = tilesx * tilesy;
    const size_t cells = static_cast<size_t>(nx) * ny;
    const unsigned short* __restrict__ cq = o.counts + static_cast<size_t>(q) * cells;
    const unsigned* __restrict__ flags = o.flags;
    unsigned long long sA[SPATIAL_MAX_SCALES] = {}, sB[SPATIAL_MAX_SCALES] = {}, sC[SPATIAL_MAX_SCALES] = {};
    unsigned n_ok = 0, n_nan = 0;

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // the same trips in every lane: uniform barriers
        const int ty = tile / tilesx, tx = tile - ty * tilesx;
        const int x0 = tx * T - H - 1, y0 = ty * T - H - 1;  // the cell of table entry (0, 0), which stays zero
        __syncthreads();  // the previous tile's reads are done (and the zeroing above)
        for (int idx = tid; idx < WW; idx += 256) {
            const int r = idx / W, c = idx - r * W;
            const int x = x0 + c, y = y0 + r;
            unsigned n = 0u, ob = 0u;
            if (r >= 1 && c >= 1 && x >= 0 && x < nx && y >= 0 && y < ny) {
                const size_t g = static_cast<size_t>(y) * nx + x;
                n = cq[g];
                ob = (flags[g] >> q) & 1u;
            }
            sn[idx] = n;
            so[idx] = static_cast<unsigned short>(ob);
        }
        __syncthreads();
        // prefix sums along the rows: waves 0, 1 the counts, waves 2, 3 the truth bits (W <= 97 rows each)
        if (tid < W) {
            unsigned acc = 0u;
            for (int c = 0; c < W; ++c) sn[tid * W + c] = acc += sn[tid * W + c];
        } else if (tid >= 128 && tid - 128 < W) {
            const int r = tid - 128;
            unsigned acc = 0u;
            for (int c = 0; c < W; ++c) so[r * W + c] = static_cast<unsigned short>(acc += so[r * W + c]);
        }
        __syncthreads();
        // then down the columns
        if (tid < W) {
            unsigned acc = 0u;
            for (int r = 0; r < W; ++r) sn[r * W + tid] = acc += sn[r * W + tid];
        } else if (tid >= 128 && tid - 128 < W) {
            const int c = tid - 128;
            unsigned acc = 0u;
            for (int r = 0; r < W; ++r) so[r * W + c] = static_cast<unsigned short>(acc += so[r * W + c]);
        }
        __syncthreads();

        for (int ci = tid; ci < T * T; ci += 256) {
            const int ly = ci / T, lx = ci - ly * T;
            const int gx = tx * T + lx, gy = ty * T + ly;
            if (gx >= nx || gy >= ny) continue;
            const size_t g = static_cast<size_t>(gy) * nx + gx;
            const unsigned fl = flags[g];
            if (fl >> 31) {
                ++n_nan;
                continue;
            }
            ++n_ok;
            atomicAdd(hist + 2 * static_cast<unsigned>(cq[g]) + ((fl >> q) & 1u), 1u);
            const int cr = ly + H + 1, cc = lx + H + 1;  // the centre's table entry
#pragma unroll
            for (int s = 0; s < SPATIAL_MAX_SCALES; ++s) {
                if (s < a.ns) {  // wave-uniform
                    const int h = a.half[s];
                    const int r0 = (cr - h - 1) * W, r1 = (cr + h) * W, c0 = cc - h - 1, c1 = cc + h;
                    const unsigned F = sn[r1 + c1] - sn[r0 + c1] - sn[r1 + c0] + sn[r0 + c0];
                    const unsigned O = static_cast<unsigned>(so[r1 + c1]) - so[r0 + c1] - so[r1 + c0] + so[r0 + c0];
                    sA[s] += static_cast<unsigned long long>(F) * F;
                    sB[s] += static_cast<unsigned long long>(O) * O;
                    sC[s] += static_cast<unsigned long long>(F) * O;
                }
            }
        }
    }

#pragma unroll
    for (int s = 0; s < SPATIAL_MAX_SCALES; ++s) {
        if (s < a.ns) {
            const unsigned long long wa = wave_sum(sA[s]), wb = wave_sum(sB[s]), wc = wave_sum(sC[s]);
            if (lane == 0) {
                atomicAdd(red + 3 * s, wa);
                atomicAdd(red + 3 * s + 1, wb);
                atomicAdd(red + 3 * s + 2, wc);
            }
        }
    }
    if (n_ok) atomicAdd(cnt, n_ok);
    if (n_nan) atomicAdd(cnt + 1, n_nan);
    __syncthreads();
    unsigned long long* table = o.table + static_cast<size_t>(q) * 2 * (M + 1);
    for (int b = tid; b < 2 * (M + 1); b += 256)
        if (hist[b]) atomicAdd(table + b, static_cast<unsigned long long>(hist[b]));
    if (tid < 3 * a.ns && red[tid]) atomicAdd(o.nbh + static_cast<size_t>(q) * 3 * a.ns + tid, red[tid]);
    if (q == 0 && tid < 2 && cnt[tid]) atomicAdd(o.cells + tid, static_cast<unsigned long long>(cnt[tid]));
}

int grid_cap(const SpatialArgs& a, int dflt) { return a.grid_max > 0 ? a.grid_max : dflt; }

bool args_ok(const EnsGeom& g, const SpatialArgs& a) {
    if (a.forecast < 1 || a.forecast > 4096 || a.nt < 1 || a.nt > VERIFY_MAX_THRESHOLDS) return false;
    if (a.ns < 0 || a.ns > SPATIAL_MAX_SCALES || a.hmax < 0 || a.hmax > SPATIAL_MAX_HALF) return false;
    for (int s = 0; s < a.ns; ++s)
        if (a.half[s] < 0 || a.half[s] > a.hmax) return false;  // a window past the halo would read outside the tables
    return a.split >= 1 && a.split <= a.forecast && a.grid_max >= 0 && a.grid_max <= 65535 &&
           static_cast<long>(g.nx) * g.ny <= (1L << 27);
}

}  // namespace

int ens_spatial_split(int cells, int forecast) {
    const int blocks = (cells + 255) / 256;
    if (blocks >= 512 || forecast < 128) return 1;  // two workgroups per CU already, or too few members to share
    return std::max(1, std::min((forecast + 63) / 64, (1024 + blocks - 1) / blocks));
}

size_t ens_spatial_lds(int forecast, int hmax) {
    const size_t ww = static_cast<size_t>(T + 2 * hmax + 1) * (T + 2 * hmax + 1);
    return SCORES_HEAD + round16(4 * ww) + round16(2 * ww) + sizeof(unsigned) * 2 * (static_cast<size_t>(forecast) + 1);
}

hipError_t ens_launch_spatial_counts(const EnsGeom& g, const double* f, const SpatialArgs& a, const SpatialOut& o,
                                     hipStream_t st) {
    if (!args_ok(g, a)) return hipErrorInvalidValue;
    const int cells = g.nx * g.ny;
    const int bx = std::min((cells + 255) / 256, grid_cap(a, SPATIAL_COUNTS_GRID_MAX));
    if (a.split == 1) {
        hipLaunchKernelGGL(k_spatial_counts<false>, dim3(bx), dim3(256), 0, st, f, g.nx, g.ny, g.pitch, g.slab, a, o);
        return hipGetLastError();
    }
    const hipError_t z = hipMemsetAsync(o.acc, 0, sizeof(unsigned) * (a.nt + 1) * static_cast<size_t>(cells), st);
    if (z != hipSuccess) return z;
    const int part = (a.forecast + a.split - 1) / a.split;
    hipLaunchKernelGGL(k_spatial_counts<true>, dim3(bx, (a.forecast + part - 1) / part), dim3(256), 0, st, f, g.nx, g.ny,
                       g.pitch, g.slab, a, o);
    hipLaunchKernelGGL(k_spatial_merge, dim3(bx), dim3(256), 0, st, f, g.nx, g.ny, g.pitch, g.slab, a, o);
    return hipGetLastError();
}

hipError_t ens_launch_spatial_scores(const EnsGeom& g, const SpatialArgs& a, const SpatialOut& o, hipStream_t st) {
    if (!args_ok(g, a)) return hipErrorInvalidValue;
    const int tiles = ((g.nx + T - 1) / T) * ((g.ny + T - 1) / T);
    const int bx = std::min(tiles, grid_cap(a, SPATIAL_SCORES_GRID_MAX));
    // the largest request: 4096 forecast members and the widest halo
    const hipError_t attr = dynamic_lds_once<k_spatial_scores>(ens_spatial_lds(4096, SPATIAL_MAX_HALF));
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(k_spatial_scores, dim3(bx, a.nt), dim3(256), ens_spatial_lds(a.forecast, a.hmax), st, g.nx, g.ny,
                       a, o);
    return hipGetLastError();
}

}  // namespace csim
