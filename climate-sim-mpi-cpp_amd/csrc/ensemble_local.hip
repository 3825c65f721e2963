// ensemble_local.hip — the local analysis of csim_ensemble_assimilate_local (host side in ensemble_analysis.cpp): every
// interior cell analysed on its own from the used observations near it, R-localised, in increasing input index; the
// text of the csim.h block.  Two launches after the screening and the inflation of the serial analysis:
//   local_prior   one wave per observation: h_{o,k} of the M forecast members to `prior` (M doubles per plan
//                 position); a point observation is its cell, a linear one obs_h<true> of obs_wave.hpp.  A
//                 screened-out observation leaves at once.  It runs apart from the update so that no cell is rewritten
//                 while an observation still reads it.
//   local_update  one wave per `pack` = G cells of one tile of the host's lookup (LocalTiles of assim_plan.hpp).  The
//                 update of a target (the cell's z, a later observation's private prior w) is a serial sum over the
//                 members, and the targets of a step are independent: targets on lanes, a loop over members.  A cell
//                 has PL = max(lmax, 1) lanes: lane 0 its z, lane s the s-th observation of its list (the first one,
//                 s = 0, is never a target and has no lane), so G <= 64 / PL cells share a wave, and the steps run to
//                 the longest list of the wave, shorter ones predicated off.
//                 z and w live in LDS member-major, T[k][column], a cell's PC = lmax + 1 columns side by side (z,
//                 observations 1 .. lmax - 1, observation 0): a lane's reads down its column are free of bank
//                 conflicts, and h'_k of the step's observation is one address per cell.  The priors arrive row by row,
//                 coalesced along k, and are transposed into T: rows are W = (G PC) | 1 doubles apart, odd, so that
//                 the transposing writes spread over the banks.
//                 A cell builds its list from its tile's entries (staged in LDS by the wave, 64 at a time) through the
//                 window, the status byte, rho > 0 and r / rho finite; a wave whose cells all have empty lists returns
//                 before it loads a member.  With one wave per SIMD (LDS: four waves per CU) nothing hides latency but
//                 the loops themselves: global loads go eight deep before their LDS writes, and the update pass reads
//                 eight members before it writes them.
// No atomics and nothing between workgroups: a cell reads and writes only itself, in place, and the priors come from
// the earlier launch.  Running sums from +0 in member order, one rounding per operation, no FMA contraction, / and
// sqrt IEEE fp64, as everywhere in ensemble_cell.hpp: the numpy restatement of the csim.h block gives the same bits.
// Only interior cells of the forecast members with a non-empty list are written.
#include <algorithm>

#include "obs_wave.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

constexpr int LOCAL_AUX = 128;                // (cell, step) entries of a wave: G PC <= 64 / PL (PL + 1) <= 128
constexpr size_t LOCAL_WAVE_LDS = 40 * 1024;  // of a wave, where more than one cell is packed: four waves per CU
constexpr size_t LOCAL_LDS_MAX = 64 * 1024;

// bytes behind T: re and y per (cell, step), the plan position per (cell, step), per cell n, i, j, and 64 entries of
// the tile's list on their way to the cells: r, y, plan position, i, j, status
constexpr size_t local_aux_bytes() {
    return (sizeof(double) * 2 + sizeof(int)) * LOCAL_AUX + sizeof(int) * 3 * 64 + (sizeof(double) * 2 + sizeof(int) * 4) * 64;
}

int local_stride(int G, int lmax) { return (G * (lmax + 1)) | 1; }

template <bool LIN>
__global__ __launch_bounds__(64) void k_local_prior(const double* __restrict__ f, int pitch, long slab, AssimArgs a,
                                                    double* __restrict__ prior) {
    extern __shared__ double sh[];  // LIN: linear_lds; else unused
    const int lane = threadIdx.x;
    const int M = a.forecast, t = a.truth_member;
    const int q = blockIdx.x;
    if (a.status && a.status[q]) return;  // screened out: the whole block, before any barrier
    double* __restrict__ out = prior + static_cast<size_t>(q) * M;
    if constexpr (LIN) {
        obs_h<true>(f, pitch, slab, a, q, sh);
        for (int k = lane; k < M; k += 64) out[k] = sh[k];
    } else {  // straight to `prior`: nothing reads the values here, so they need no LDS and no barrier
        const double* p = cell_ptr(f, a.obs.i[q], a.obs.j[q], pitch);
        for (int k = lane; k < M; k += 64) out[k] = p[static_cast<ptrdiff_t>(forecast_member(k, t)) * slab];
    }
}

__global__ __launch_bounds__(64) void k_local_update(double* __restrict__ f, int nx, int ny, int pitch, long slab,
                                                     AssimArgs a, LocalArgs l, int passes, int W) {
    extern __shared__ __attribute__((aligned(16))) double T[];  // [M][W], then the aux arrays
    const int lane = threadIdx.x;
    const int M = a.forecast, t = a.truth_member;
    const int G = l.pack, PL = max(l.lmax, 1), PC = l.lmax + 1;
    double* sre = T + static_cast<size_t>(M) * W;  // re of (cell, step) at g PC + o
    double* sy = sre + LOCAL_AUX;                  // y
    int* sq = reinterpret_cast<int*>(sy + LOCAL_AUX);  // plan position
    int* sn = sq + LOCAL_AUX;                      // per cell: the length of its list, then (i, j)
    int* sci = sn + 64;
    int* scj = sci + 64;

    double* er = reinterpret_cast<double*>(scj + 64);  // 64 entries of the tile's list: r, y, plan position, i, j, status
    double* ey = er + 64;
    int* eq = reinterpret_cast<int*>(ey + 64);
    int* ei = eq + 64;
    int* ej = ei + 64;
    int* es = ej + 64;

    const int tileid = blockIdx.x / passes, pass = blockIdx.x - tileid * passes;
    const int ty = tileid / l.ntx, tx = tileid - ty * l.ntx;
    const int g = lane / PL, slot = lane - g * PL;
    const bool lane_on = g < G;
    // the list of the cell, by its first lane: the tile's entries in input order, through the window, the status byte,
    // rho > 0 and r / rho finite.  At most lmax pass the window (the host's bound), so the list fits.  The wave brings
    // the entries in 64 at a time, one per lane, so that a cell's walk over them reads LDS
    const int cidx = pass * G + g;  // the cell of the tile, row-major
    const int cr = cidx / l.tile, cc = cidx - cr * l.tile;
    const int ci = tx * l.tile + cc + 1, cj = ty * l.tile + cr + 1;
    const bool lists = lane_on && slot == 0 && cr < l.tile && ci <= nx && cj <= ny;
    const int c0 = l.cstart[tileid], c1 = l.cstart[tileid + 1];
    int n = 0;
    sn[lane] = 0;
    __syncthreads();
    for (int base = c0; base < c1; base += 64) {
        __syncthreads();  // the walks over the last 64 are done
        if (base + lane < c1) {
            const int q = l.cpos[base + lane];
            eq[lane] = q, ei[lane] = a.obs.i[q], ej[lane] = a.obs.j[q];
            es[lane] = a.status ? a.status[q] : 0;
            er[lane] = a.obs.r[q], ey[lane] = a.obs.y[q];
        }
        __syncthreads();
        const int m = min(64, c1 - base);
        if (lists)
            for (int u = 0; u < m && n < l.lmax; ++u) {
                const int di = ci - ei[u], dj = cj - ej[u];
                if (abs(di) > a.lx || abs(dj) > a.ly || es[u]) continue;
                const double rho = window_rho(a.rho, a.lx, a.ly, di, dj);
                if (!(rho > 0.0)) continue;
                const double re = er[u] / rho;
                if (!__builtin_isfinite(re)) continue;
                sq[g * PC + n] = eq[u];
                sre[g * PC + n] = re;
                sy[g * PC + n] = ey[u];
                ++n;
            }
    }
    if (lists) sn[g] = n, sci[g] = ci, scj[g] = cj;
    __syncthreads();
    const int ng = lane_on ? sn[g] : 0;
    int S = ng;  // the steps of the wave: its longest list
    for (int h = 32; h >= 1; h >>= 1) S = max(S, __shfl_xor(S, h));
    if (S == 0) return;  // the same in every lane

    // z: cell g of member k is element k G + g, so a load takes the G cells of a member side by side.  Eight loads are
    // in flight before the first is stored, here and for the priors below
    {
        const int dk = 64 / G, dg = 64 - dk * G;  // what 64 elements further means for (k, g)
        const int total = M * G;
        int k = lane / G, c = lane - k * G;
        for (int e0 = lane; e0 < total; e0 += 8 * 64) {
            double v[8];
            int at[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool ok = e0 + 64 * u < total && sn[c] > 0;
                at[u] = ok ? k * W + c * PC : -1;
                v[u] = ok ? cell_ptr(f, sci[c], scj[c], pitch)[static_cast<ptrdiff_t>(forecast_member(k, t)) * slab] : 0.0;
                k += dk, c += dg;
                if (c >= G) c -= G, ++k;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (at[u] >= 0) T[at[u]] = v[u];
        }
    }
    // w: entry rs = c PC + s is the s-th observation of cell c; its prior, a row along k, goes into column
    // c PC + (s ? s : lmax)
    for (int k0 = 0; k0 < M; k0 += 64) {
        const int k = k0 + lane;
        for (int rs0 = 0; rs0 < G * PC; rs0 += 8) {
            double v[8];
            int at[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int rs = rs0 + u, c = rs / PC, s = rs - c * PC;
                const bool ok = rs < G * PC && s < sn[c] && k < M;
                at[u] = ok ? k * W + c * PC + (s ? s : l.lmax) : -1;
                v[u] = ok ? l.prior[static_cast<size_t>(sq[rs]) * M + k] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (at[u] >= 0) T[at[u]] = v[u];
        }
    }
    __syncthreads();

    const double dM = static_cast<double>(M), dM1 = static_cast<double>(M - 1);
    const double* own = T + (lane_on ? g * PC + slot : 0);  // lanes without a cell read column 0 and write nothing
    double* own_w = T + (lane_on ? g * PC + slot : 0);
    const int gc = lane_on ? g : 0;
    for (int o = 0; o < S; ++o) {
        const bool step = o < ng;  // this cell still has an observation
        const bool target = step && (slot == 0 || (slot > o && slot < ng));  // z, and the observations after o
        const double* hcol = T + (step ? gc * PC + (o ? o : l.lmax) : 0);
        const double re = sre[step ? gc * PC + o : 0], y = sy[step ? gc * PC + o : 0];
        double sh = 0.0, sv = 0.0;
#pragma unroll 8
        for (int k = 0; k < M; ++k) {
            sh = sh + hcol[static_cast<size_t>(k) * W];
            sv = sv + own[static_cast<size_t>(k) * W];
        }
        const double hbar = sh / dM, vbar = sv / dM;
        double pp = 0.0, cc = 0.0;
#pragma unroll 8
        for (int k = 0; k < M; ++k) {
            const double hp = hcol[static_cast<size_t>(k) * W] - hbar;
            pp = pp + hp * hp;
            cc = cc + (own[static_cast<size_t>(k) * W] - vbar) * hp;
        }
        const double d = pp / dM1 + re;
        const double alpha = 1.0 / (1.0 + sqrt(re / d));
        const double delta = y - hbar;
        const double gain = (cc / dM1) / d;
        const double beta = alpha * gain;
        const double gd = gain * delta;
        // no lane writes a column that another reads in this step: the step's observation is no target.  Eight members
        // are read before the first is written, so that the writes do not put an LDS round trip between the reads
        if (target) {
            int k = 0;
            for (; k + 8 <= M; k += 8) {
                double h[8], v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    h[u] = hcol[static_cast<size_t>(k + u) * W];
                    v[u] = own[static_cast<size_t>(k + u) * W];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) own_w[static_cast<size_t>(k + u) * W] = v[u] + (gd - beta * (h[u] - hbar));
            }
            for (; k < M; ++k) {
                const double hp = hcol[static_cast<size_t>(k) * W] - hbar;
                own_w[static_cast<size_t>(k) * W] = own[static_cast<size_t>(k) * W] + (gd - beta * hp);
            }
        }
        __syncthreads();  // the next step's observation was a target of this one
    }

    {
        const int dk = 64 / G, dg = 64 - dk * G;
        int k = lane / G, c = lane - k * G;
        for (int e = lane; e < M * G; e += 64) {
            if (sn[c] > 0)
                cell_ptr(f, sci[c], scj[c], pitch)[static_cast<ptrdiff_t>(forecast_member(k, t)) * slab] =
                    T[static_cast<size_t>(k) * W + c * PC];
            k += dk, c += dg;
            if (c >= G) c -= G, ++k;
        }
    }
}

}  // namespace

int ens_local_pack(int M, int lmax, int want) {
    const int PL = std::max(lmax, 1);
    int G = 64 / PL;
    if (want > 0) G = std::min(G, want);
    while (G > 1 && sizeof(double) * M * local_stride(G, lmax) + local_aux_bytes() > LOCAL_WAVE_LDS) --G;
    return std::max(G, 1);
}

hipError_t ens_launch_local_prior(const EnsGeom& g, const double* f, const AssimArgs& a, int nobs, double* prior,
                                  hipStream_t st) {
    if (nobs <= 0) return hipSuccess;
    if (a.forecast < 2 || a.forecast > ASSIM_MAX_MEMBERS) return hipErrorInvalidValue;
    return for_obs_form(a, 0, [&](auto lin, size_t lds) {
        hipLaunchKernelGGL(k_local_prior<decltype(lin)::value>, dim3(nobs), dim3(64), lds, st, f, g.pitch, g.slab, a,
                           prior);
        return hipGetLastError();
    });
}

hipError_t ens_launch_local_update(const EnsGeom& g, double* f, const AssimArgs& a, const LocalArgs& l, hipStream_t st) {
    const int M = a.forecast;
    if (M < 2 || M > ASSIM_MAX_MEMBERS || l.lmax < 0 || l.lmax > LOCAL_MAX_OBS ||
        static_cast<long>(l.lmax) * M > LOCAL_MAX_DOUBLES)
        return hipErrorInvalidValue;
    if (l.lmax == 0) return hipSuccess;  // no cell has an observation
    if ((l.tile != 4 && l.tile != 8 && l.tile != 16) || l.pack < 1 || l.pack > 64 / std::max(l.lmax, 1))
        return hipErrorInvalidValue;
    const int W = local_stride(l.pack, l.lmax);
    const size_t lds = sizeof(double) * M * W + local_aux_bytes();
    if (lds > LOCAL_LDS_MAX) return hipErrorInvalidValue;
    const int passes = (l.tile * l.tile + l.pack - 1) / l.pack;
    const long blocks = static_cast<long>(l.ntx) * l.nty * passes;
    if (blocks <= 0 || blocks > 0x7fffffffL) return hipErrorInvalidValue;
    if (hipError_t err = dynamic_lds_once<k_local_update>(LOCAL_LDS_MAX)) return err;
    hipLaunchKernelGGL(k_local_update, dim3(static_cast<unsigned>(blocks)), dim3(64), lds, st, f, g.nx, g.ny, g.pitch,
                       g.slab, a, l, passes, W);
    return hipGetLastError();
}

}  // namespace csim
