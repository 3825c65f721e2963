// ensemble_letkf.hip — the two kernels of csim_ensemble_assimilate_letkf that make the ETKF local (host side in
// ensemble_analysis.cpp; the definition is the LETKF block of csim.h; the lattice of nodes is letkf_nodes.hpp).  Between them
// run the batched eigensolver and the batched weights of sym_eigen_device.hip.
//   k_letkf_gram   Workgroup (g, y) of 256 lanes serves node g: A_g = Z^T Z over L(g), the used observations whose
//                  window holds the node's cell, with the localisation in the observation error.  The node's
//                  candidates (the host's lookup, sorted by input index) come 64 at a time, one per lane: the status
//                  byte, rho > 0 and r / rho finite decide, and the ones that pass are packed to the front in their
//                  order, so that the running sums have exactly L(g)'s terms.  Their priors h_{o,k} arrive row by row,
//                  coalesced along k, into LDS as [observation][member]; 64 lanes form hb, the rows are normalised with
//                  sqrt(r / rho), z_M goes to column M, and the GramTile of gram_tile.hpp walks the rows: the node is one
//                  class, and the lanes' sums are carried from one 64 to the next.  A chunk without a local observation
//                  costs its status bytes and nothing else.
//   k_letkf_cells  The cells between four nodes, a patch, share the four W: a workgroup takes 64 cells of one patch,
//                  one per lane, its p_k held and applied by espace_cell.hpp as in k_espace_apply: in registers (P > 0,
//                  the steps of for_step) or in LDS (P = 0: M > 64, or letkf_form 1).  The status of a node is read
//                  with a wave-uniform address like its W and wbar.  A node whose weight is zero at a lane's cell takes
//                  no part there; a node that is IDLE or NONFINITE stands for the identity.  A member's value is written
//                  once all M have been read.
// Every product and every sum is one rounded fp64 operation, no FMA contraction; / and sqrt are IEEE fp64.
#include <algorithm>

#include "espace_cell.hpp"
#include "gram_tile.hpp"
#include "letkf_nodes.hpp"
#include "obs_wave.hpp"

#pragma clang fp contract(off)

namespace csim {

namespace {

// dynamic LDS of k_letkf_gram: the rows, then sqrt(re), y and hb of the chunk's rows and their plan positions
inline size_t lg_lds(int M) {
    return sizeof(double) * (static_cast<size_t>(GRAM_SEG) * gram_stride(M + 1) + 3 * GRAM_SEG) + sizeof(int) * GRAM_SEG;
}

template <int NB>
__global__ __launch_bounds__(GRAM_THREADS) void k_letkf_gram(int nx, int ny, AssimArgs a, LetkfGramArgs l) {
    extern __shared__ __attribute__((aligned(16))) double held[];  // [64][stride], then sre, y, hb, q
    const int M = a.forecast, MA = M + 1;
    const int stride = gram_stride(MA);
    double* __restrict__ sres = held + GRAM_SEG * stride;
    double* __restrict__ ys = sres + GRAM_SEG;
    double* __restrict__ hbs = ys + GRAM_SEG;
    int* __restrict__ qs = reinterpret_cast<int*>(hbs + GRAM_SEG);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mpad = gram_nblk(MA) * GRAM_TB;
    const int node = blockIdx.x;
    const int nb = node / l.nax, na = node - nb * l.nax;
    const int ci = letkf_node_at(na, l.spacing, nx), cj = letkf_node_at(nb, l.spacing, ny);
    GramTile<NB> tile;
    tile.init(MA);
    int cnt = 0;

    const int c0 = l.cstart[node], c1 = l.cstart[node + 1];
    for (int base = c0; base < c1; base += GRAM_SEG) {
        // every wave looks at the same 64 candidates, so the count below is the workgroup's
        bool used = false;
        int q = 0;
        double re = 0.0;
        if (base + lane < c1) {
            q = l.cpos[base + lane];
            if (!(a.status && a.status[q])) {
                const int di = ci - a.obs.i[q], dj = cj - a.obs.j[q];
                if (abs(di) <= a.lx && abs(dj) <= a.ly) {
                    const double rho = window_rho(a.rho, a.lx, a.ly, di, dj);
                    if (rho > 0.0) {
                        re = a.obs.r[q] / rho;
                        used = __builtin_isfinite(re);
                    }
                }
            }
        }
        const unsigned long long pass = __ballot(used);
        const int nc = __popcll(pass);
        if (nc == 0) continue;
        if (wave == 0 && used) {
            const int row = __popcll(pass & ((1ull << lane) - 1ull));
            qs[row] = q, sres[row] = sqrt(re), ys[row] = a.obs.y[q];
        }
        __syncthreads();
        for (int r = wave; r < nc; r += GRAM_THREADS / 64) {
            const double* __restrict__ h = l.prior + static_cast<size_t>(qs[r]) * M;
            double* __restrict__ row = held + r * stride;
            for (int k = lane; k < M; k += 64) row[k] = h[k];
            for (int k = MA + lane; k < mpad; k += 64) row[k] = 0.0;
        }
        __syncthreads();
        if (tid < nc) hbs[tid] = gram_row_mean(held + tid * stride, M);
        __syncthreads();
        for (int r = wave; r < nc; r += GRAM_THREADS / 64) {
            double* __restrict__ row = held + r * stride;
            const double hb = hbs[r], sr = sres[r];
            for (int k = lane; k < M; k += 64) row[k] = (row[k] - hb) / sr;
            if (lane == 0) row[M] = (ys[r] - hb) / sr;
        }
        __syncthreads();
        tile.walk(held, stride, nc);
        __syncthreads();
        cnt += nc;
    }
    // the node's sums as the full matrix, mirrored: the eigensolver and the weights read A where it lies
    double* __restrict__ A = l.A + static_cast<size_t>(node) * MA * MA;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if (!tile.mine[u]) continue;
#pragma unroll
        for (int i = 0; i < GRAM_TB; ++i)
#pragma unroll
            for (int j = 0; j < GRAM_TB; ++j) {
                const int ra = GRAM_TB * tile.ia[u] + i, rb = GRAM_TB * tile.ib[u] + j;
                if (ra <= rb && rb < MA) {
                    const double s = tile.acc[u][i * GRAM_TB + j];
                    A[static_cast<size_t>(ra) * MA + rb] = s;
                    A[static_cast<size_t>(rb) * MA + ra] = s;
                }
            }
    }
    if (blockIdx.y == 0 && tid == 0) l.count[node] = cnt;
}

__device__ __forceinline__ bool letkf_active(int status) { return status == LETKF_OK || status == LETKF_NOT_CONVERGED; }

// grid: patches x chunks; chunk c of a patch holds its cells 64 c .. 64 c + 63, row-major within the patch
template <int P>
__global__ __launch_bounds__(P > 0 ? 64 : 64 * CELL_WAVES) void k_letkf_cells(
    double* __restrict__ f, int nx, int ny, int pitch, long slab, int M, int t, int nax, int nay, int spacing,
    int chunks, const double* __restrict__ Wall, const double* __restrict__ wbarall, const int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double held[];  // P = 0: [M][64]
    constexpr int NW = P > 0 ? 1 : CELL_WAVES;
    const int lane = threadIdx.x & 63, wave = P > 0 ? 0 : threadIdx.x >> 6;
    const int npx = max(nax - 1, 1), npy = max(nay - 1, 1);
    const int patch = blockIdx.x / chunks, chunk = blockIdx.x - patch * chunks;
    const int pb = patch / npx, pa = patch - pb * npx;
    const int i0 = letkf_node_at(pa, spacing, nx), j0 = letkf_node_at(pb, spacing, ny);
    const int i1 = pa == npx - 1 ? nx : letkf_node_at(pa + 1, spacing, nx) - 1;
    const int j1 = pb == npy - 1 ? ny : letkf_node_at(pb + 1, spacing, ny) - 1;
    const int pw = i1 - i0 + 1, pcells = pw * (j1 - j0 + 1);
    if (chunk * 64 >= pcells) return;  // this patch is smaller than the largest: the whole workgroup
    // the four nodes; along an axis with one node both are that node, and the second has weight +0
    const int pa1 = min(pa + 1, nax - 1), pb1 = min(pb + 1, nay - 1);
    const int nd[4] = {pb * nax + pa, pb * nax + pa1, pb1 * nax + pa, pb1 * nax + pa1};
    bool act[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) act[n] = letkf_active(status[nd[n]]);
    if (!(act[0] || act[1] || act[2] || act[3])) return;  // no cell of the patch is written
    const bool idle = !(act[0] && act[1] && act[2] && act[3]);

    const int e = chunk * 64 + lane;
    const bool valid = e < pcells;  // a lane past the end works on the last cell and stores nothing
    const int ec = valid ? e : pcells - 1;
    const int rj = ec / pw, ri = ec - rj * pw;
    const int i = i0 + ri, j = j0 + rj;
    double beta[4];
    letkf_weights4(letkf_axis_blend(i, spacing, nx, nax).t, letkf_axis_blend(j, spacing, ny, nay).t, beta);
    bool use[4], write = false;
#pragma unroll
    for (int n = 0; n < 4; ++n) use[n] = beta[n] != 0.0, write = write || (use[n] && act[n]);
    write = write && valid;

    double* __restrict__ p = cell_ptr(f, i, j, pitch);
    double x[P > 0 ? P : 1];
    const double m = cell_hold<P>(p, slab, M, t, true, lane, wave, x, held);
    const size_t mm = static_cast<size_t>(M) * M;
    double d[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        if (!act[n]) continue;  // the same in every lane
        d[n] = cell_dot<P>(x, held, lane, M, wbarall + static_cast<size_t>(nd[n]) * M);
    }
    for (int r0 = CELL_RB * wave; r0 < M; r0 += CELL_RB * NW) {
        int rr[CELL_RB];
        double c[CELL_RB], pr[CELL_RB];
#pragma unroll
        for (int u = 0; u < CELL_RB; ++u) rr[u] = min(r0 + u, M - 1), c[u] = 0.0, pr[u] = 0.0;
        if (idle) {
            // p_r of the outputs, for the nodes that stand for the identity: the register form reads the members again
            // (the same bits; they are written further down), the LDS form has them at hand
#pragma unroll
            for (int u = 0; u < CELL_RB; ++u) {
                if constexpr (P > 0)
                    pr[u] = p[static_cast<size_t>(forecast_member(rr[u], t)) * slab] - m;
                else
                    pr[u] = held[rr[u] * 64 + lane];
            }
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            double s[CELL_RB];
            if (act[n]) {
#pragma unroll
                for (int u = 0; u < CELL_RB; ++u) s[u] = 0.0;
                const double* __restrict__ W = Wall + static_cast<size_t>(nd[n]) * mm;
                CSIM_CELL_APPLY(P, x, held, lane, M, W, M, rr, s)
            } else {
#pragma unroll
                for (int u = 0; u < CELL_RB; ++u) s[u] = pr[u];
            }
            if (use[n]) {
#pragma unroll
                for (int u = 0; u < CELL_RB; ++u) c[u] = c[u] + beta[n] * (d[n] + s[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < CELL_RB; ++u)
            if (r0 + u < M && write) p[static_cast<size_t>(forecast_member(r0 + u, t)) * slab] = m + c[u];
    }
}

}  // namespace

hipError_t ens_launch_letkf_gram(const EnsGeom& g, const AssimArgs& a, const LetkfGramArgs& l, int form, hipStream_t st) {
    const int M = a.forecast, MA = M + 1;
    const long nodes = static_cast<long>(l.nax) * l.nay;
    if (M < 2 || M > ESPACE_MAX_MEMBERS || l.spacing < 1 || nodes < 1 || nodes > LETKF_MAX_NODES || form < 0 ||
        form > GRAM_FORMS)
        return hipErrorInvalidValue;
    return for_gram_form(form, M, [&](auto nb) {
        constexpr int NB = decltype(nb)::value;
        const hipError_t attr = dynamic_lds_once<k_letkf_gram<NB>>(lg_lds(ESPACE_MAX_MEMBERS));
        if (attr != hipSuccess) return attr;
        hipLaunchKernelGGL(k_letkf_gram<NB>, dim3(static_cast<unsigned>(nodes), gram_shares(MA, NB)), dim3(GRAM_THREADS),
                           lg_lds(M), st, g.nx, g.ny, a, l);
        return hipGetLastError();
    });
}

hipError_t ens_launch_letkf_cells(const EnsGeom& g, double* f, int M, int t, const LetkfCellArgs& l, int form,
                                  hipStream_t st) {
    const long nodes = static_cast<long>(l.nax) * l.nay;
    if (M < 2 || M > ESPACE_MAX_MEMBERS || l.spacing < 1 || nodes < 1 || nodes > LETKF_MAX_NODES || form < 0 ||
        form > LETKF_FORMS || l.nax != letkf_axis_nodes(g.nx, l.spacing) || l.nay != letkf_axis_nodes(g.ny, l.spacing))
        return hipErrorInvalidValue;
    // the widest and the tallest patch: the first one, or the last one, which also holds the last node's cells
    auto longest = [](int n, int s, int na) {
        if (na < 2) return 1;
        const int last = n - letkf_node_at(na - 2, s, n) + 1;
        return na > 2 ? std::max(last, s) : last;
    };
    const long pmax = static_cast<long>(longest(g.nx, l.spacing, l.nax)) * longest(g.ny, l.spacing, l.nay);
    const long chunks = (pmax + 63) / 64;
    const long blocks = static_cast<long>(std::max(l.nax - 1, 1)) * std::max(l.nay - 1, 1) * chunks;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    auto launch = [&](auto s) {
        constexpr int P = decltype(s)::value;
        const size_t lds = P > 0 ? 0 : sizeof(double) * 64 * static_cast<size_t>(M);
        if (P == 0) {
            const hipError_t attr = dynamic_lds_once<k_letkf_cells<P>>(sizeof(double) * 64 * ESPACE_MAX_MEMBERS);
            if (attr != hipSuccess) return attr;
        }
        hipLaunchKernelGGL(k_letkf_cells<P>, dim3(static_cast<unsigned>(blocks)), dim3(P > 0 ? 64 : 64 * CELL_WAVES), lds,
                           st, f, g.nx, g.ny, g.pitch, g.slab, M, t, l.nax, l.nay, l.spacing, static_cast<int>(chunks),
                           l.W, l.wbar, l.status);
        return hipGetLastError();
    };
    if (form == 1) return launch(Step<0>{});
    return for_step(M, launch);
}

}  // namespace csim
