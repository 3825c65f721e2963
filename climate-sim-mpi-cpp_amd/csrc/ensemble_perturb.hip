// ensemble_perturb.hip — the kernel of csim_ensemble_perturb (host side in ensemble_da.cpp): x_k += sigma p_k on every
// interior cell of the forecast members, p_k a smoothed white-noise field that is a pure function of (seed, draw,
// member, cell), as include/csim.h defines it.  Needs only the slab layout of ensemble.hpp and ensemble_noise.hpp.
//
// One launch, no global scratch.  A workgroup of 256 threads owns a tile of 64 x TY interior cells (blockIdx.x) and a
// share of the forecast members (blockIdx.y: members y, y + gridDim.y, ...).  Per member it
//   1. fills an LDS tile of (TY + 2 ry) x (64 + 2 rx) lattice points with white noise.  The noise is counter based, so
//      the aprons of neighbouring tiles regenerate the same values.  One Philox call yields the deviates of the lattice
//      points 2n and 2n + 1: a work item is a pair of neighbouring tile slots aligned on that parity, and calls Philox a
//      second time only where a periodic wrap puts its two slots into different calls;
//   2. smooths along x into a second LDS tile of (TY + 2 ry) x 64 (lanes follow i: conflict-free reads);
//   3. smooths along y into registers (TY / 4 cells per thread) and does the one read-modify-write of the member.
// centered: the workgroup first runs 1 - 3 over all M forecast members to form the running sum of p_k in member order in
// registers, then regenerates p_k for its own members; workgroups of one tile repeat that sum, which is the price of
// keeping its order without a second kernel and a scratch field (the host gives centered calls fewer member shares).
// Every sum is a running sum from +0 in the order of csim.h, every product rounded, no FMA contraction; the result does
// not depend on TY, on the member shares or on the tile a cell falls into.  Only interior cells of the forecast members
// are written; ghost rings, member t and the other ping-pong buffer are never touched.
#include <algorithm>

#include "ensemble.hpp"
#include "ensemble_noise.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr int PERTURB_TX = 64;

struct PerturbTile {
    int x0, y0;    // the tile's first interior cell is (x0 + 1, y0 + 1)
    int tw, th;    // its cells (clipped to the interior)
    int W, HR;     // its lattice points: tw + 2 rx, th + 2 ry
    int WS;        // row stride of the white-noise tile: 64 + 2 rx
    int NP;        // work items per lattice row
    int nx, ny;
    long long Px;  // lattice points per lattice row
};

// the deviate of lattice point L from the Philox output of L >> 1
__device__ __forceinline__ double perturb_pick(const unsigned (&o)[4], long long L) {
    const int s = static_cast<int>(L & 1);
    return normal_from_bits(static_cast<unsigned long long>(o[2 * s]) |
                            (static_cast<unsigned long long>(o[2 * s + 1]) << 32));
}

__device__ __forceinline__ void perturb_call(unsigned (&o)[4], long long L, unsigned member, const PerturbArgs& a) {
    const unsigned long long n = static_cast<unsigned long long>(L) >> 1;
    o[0] = static_cast<unsigned>(n), o[1] = static_cast<unsigned>(n >> 32), o[2] = member, o[3] = a.draw;
    philox4x32(o, a.seed_lo, a.seed_hi);
}

// p[m] = p_member at the thread's cells (column tid & 63, rows (tid >> 6) + 4 m of the tile); 0 outside the tile
template <int TY>
__device__ __forceinline__ void perturb_field(const PerturbArgs& a, const PerturbTile& t, unsigned member,
                                              double* __restrict__ w, double* __restrict__ hx,
                                              double (&p)[TY / 4]) {
    const int tid = threadIdx.x;
    const int rx = a.rx, ry = a.ry;
    // 1. white noise
    for (int it = tid; it < t.HR * t.NP; it += 256) {
        const int r = it / t.NP, q = it - r * t.NP;
        const int b = a.pery ? (t.y0 + r - ry + t.ny) % t.ny : t.y0 + r;
        const long long row = static_cast<long long>(b) * t.Px;
        auto col = [&](int c) { return a.perx ? (t.x0 + c - rx + t.nx) % t.nx : t.x0 + c; };
        const int par = static_cast<int>((row + col(0)) & 1);
        const int c0 = 2 * q - par, c1 = c0 + 1;
        const bool ok0 = c0 >= 0 && c0 < t.W, ok1 = c1 < t.W;
        if (!ok0 && !ok1) continue;
        const long long L1 = row + col(ok1 ? c1 : c0);
        const long long L0 = ok0 ? row + col(c0) : L1;
        unsigned o[4];
        perturb_call(o, L0, member, a);
        if (ok0) w[r * t.WS + c0] = perturb_pick(o, L0);
        if (ok1) {
            if ((L1 >> 1) != (L0 >> 1)) perturb_call(o, L1, member, a);
            w[r * t.WS + c1] = perturb_pick(o, L1);
        }
    }
    __syncthreads();
    // 2. along x
    const int i = tid & 63;
    if (i < t.tw)
        for (int r = tid >> 6; r < t.HR; r += 4) {
            const double* src = w + r * t.WS + i;
            double s = 0.0;
            for (int o = 0; o <= 2 * rx; ++o) s = s + a.tx[o] * src[o];
            hx[r * PERTURB_TX + i] = s;
        }
    __syncthreads();
    // 3. along y
#pragma unroll
    for (int m = 0; m < TY / 4; ++m) {
        const int jj = (tid >> 6) + 4 * m;
        double s = 0.0;
        if (i < t.tw && jj < t.th) {
            const double* src = hx + jj * PERTURB_TX + i;
            for (int o = 0; o <= 2 * ry; ++o) s = s + a.ty[o] * src[o * PERTURB_TX];
        }
        p[m] = s;
    }
}

template <int TY, bool CENTERED>
__global__ __launch_bounds__(256) void k_ensemble_perturb(double* __restrict__ f, int nx, int ny, int pitch, long slab,
                                                          int tiles_x, PerturbArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sh[];
    PerturbTile t;
    t.x0 = static_cast<int>(blockIdx.x % tiles_x) * PERTURB_TX;
    t.y0 = static_cast<int>(blockIdx.x / tiles_x) * TY;
    t.tw = min(PERTURB_TX, nx - t.x0), t.th = min(TY, ny - t.y0);
    t.W = t.tw + 2 * a.rx, t.HR = t.th + 2 * a.ry;
    t.WS = PERTURB_TX + 2 * a.rx;
    t.NP = t.W / 2 + 1;
    t.nx = nx, t.ny = ny;
    t.Px = a.perx ? nx : nx + 2 * a.rx;
    double* w = sh;                           // (TY + 2 ry) x WS
    double* hx = sh + (TY + 2 * a.ry) * t.WS;  // (TY + 2 ry) x 64
    const int M = a.forecast;
    const int tid = threadIdx.x, i = tid & 63;
    double p[TY / 4], pbar[TY / 4];
    if (CENTERED) {
        double acc[TY / 4];
#pragma unroll
        for (int m = 0; m < TY / 4; ++m) acc[m] = 0.0;
        for (int k = 0; k < M; ++k) {
            perturb_field<TY>(a, t, static_cast<unsigned>(k + (k >= a.truth_member)), w, hx, p);
#pragma unroll
            for (int m = 0; m < TY / 4; ++m) acc[m] = acc[m] + p[m];
        }
        const double den = static_cast<double>(M);
#pragma unroll
        for (int m = 0; m < TY / 4; ++m) pbar[m] = acc[m] / den;
    }
    for (int k = blockIdx.y; k < M; k += gridDim.y) {
        const int member = k + (k >= a.truth_member);
        perturb_field<TY>(a, t, static_cast<unsigned>(member), w, hx, p);
        if (i >= t.tw) continue;  // no barrier depends on what follows
        double* fm = f + static_cast<ptrdiff_t>(member) * slab;
#pragma unroll
        for (int m = 0; m < TY / 4; ++m) {
            const int jj = (tid >> 6) + 4 * m;
            if (jj >= t.th) continue;
            double* c = fm + static_cast<ptrdiff_t>(t.y0 + jj + 1) * pitch + (LPAD - 1) + (t.x0 + i + 1);
            const double v = CENTERED ? p[m] - pbar[m] : p[m];
            *c = *c + a.sigma * v;
        }
    }
}

template <int TY, bool CENTERED>
hipError_t launch_perturb(const EnsGeom& g, double* f, const PerturbArgs& a, int shares, hipStream_t st) {
    constexpr int lds_max = static_cast<int>(sizeof(double)) * (TY + 2 * PERTURB_MAX_RADIUS) *
                            (2 * PERTURB_TX + 2 * PERTURB_MAX_RADIUS);
    static_assert(lds_max <= 160 * 1024, "the tiles of the largest radius must fit the LDS");
    static const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(k_ensemble_perturb<TY, CENTERED>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    if (attr != hipSuccess) return attr;
    const int tiles_x = (g.nx + PERTURB_TX - 1) / PERTURB_TX, tiles_y = (g.ny + TY - 1) / TY;
    const size_t lds = sizeof(double) * static_cast<size_t>(TY + 2 * a.ry) * (2 * PERTURB_TX + 2 * a.rx);
    hipLaunchKernelGGL((k_ensemble_perturb<TY, CENTERED>), dim3(static_cast<unsigned>(tiles_x) * tiles_y, shares),
                       dim3(256), lds, st, f, g.nx, g.ny, g.pitch, g.slab, tiles_x, a);
    return hipGetLastError();
}

}  // namespace

hipError_t ens_launch_perturb(const EnsGeom& g, double* f, const PerturbArgs& a, bool centered, hipStream_t st,
                              int tile_rows, int member_shares) {
    if (a.rx < 0 || a.ry < 0 || a.rx > PERTURB_MAX_RADIUS || a.ry > PERTURB_MAX_RADIUS || a.forecast < 1)
        return hipErrorInvalidValue;
    if ((tile_rows != 0 && tile_rows != 8 && tile_rows != 32) || member_shares < 0 || member_shares > 65535)
        return hipErrorInvalidValue;
    if (static_cast<long long>((g.nx + PERTURB_TX - 1) / PERTURB_TX) * ((g.ny + 7) / 8) > 0x7fffffffLL)
        return hipErrorInvalidValue;
    // Tiles of 32 rows regenerate the least apron; tiles of 8 rows give a small grid four times the workgroups.  The
    // member shares then fill the machine: about 2048 workgroups, or, centered, 512, as every share repeats the sum
    // over all members (M + M / shares fields per workgroup).  The options perturb_tile_rows and
    // perturb_member_shares (tests) replace either choice; 0 keeps it.
    const long tiles32 = static_cast<long>((g.nx + PERTURB_TX - 1) / PERTURB_TX) * ((g.ny + 31) / 32);
    const long want = centered ? 512 : 2048;
    const bool tall = tile_rows ? tile_rows == 32 : tiles32 * (centered ? 1 : a.forecast) >= want / 2;
    const long tiles = tall ? tiles32 : static_cast<long>((g.nx + PERTURB_TX - 1) / PERTURB_TX) * ((g.ny + 7) / 8);
    const int shares =
        member_shares ? std::min(member_shares, a.forecast)
                      : static_cast<int>(std::max(1L, std::min<long>({(want + tiles - 1) / tiles, a.forecast, 65535L})));
    if (tall)
        return centered ? launch_perturb<32, true>(g, f, a, shares, st) : launch_perturb<32, false>(g, f, a, shares, st);
    return centered ? launch_perturb<8, true>(g, f, a, shares, st) : launch_perturb<8, false>(g, f, a, shares, st);
}

}  // namespace csim
