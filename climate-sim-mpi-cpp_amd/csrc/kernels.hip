// kernels.hip — the main translation unit of the hand-written gfx950 (CDNA4, wave64) kernels of the
// advection–diffusion hot path: everything but the default fused sweep, and every launch_* entry.
//
// Kernels, in file order: k_sweep_dpp (1 step/pass), k_sweep_lds (the LDS-staged design, measured
// alternative), k_sweep_naive (strawman), then the small kernels (ghost fill / extend, edge and face
// packing, reference-granularity operators, reductions, the bit-identity checksum).  k_sweepO_dpp
// (2-7 steps/pass, overlapped strips, DEFAULT) lives in sweepO.hpp and is compiled once per depth
// (sweepO_inst.hip); the device code it shares with this file and with ensemble.hip is sweep_core.hpp.
#include "sweep_core.hpp"

#pragma clang fp contract(off)

namespace csim {

// The six instantiations sweepO_T<2..7> (sweepO.hpp) — 60 kernels with two bodies each, 90 % of the library's
// compile time — are six translation units of their own (sweepO_inst.hip), built in parallel with this one, which
// only declares the template: launch_sweepO below links against them.
template <int T>
hipError_t sweepO_T(const double* in, double* out, int pitch, const Phys& p, const SweepCfg& cfg, const Bc2& bc,
                    const FinLines& fin, const SweepPlan& plan, hipStream_t st, const FrameSync& fs, const unsigned* lease);
// ... and two more for the plans with wide strips (sweepO_wide_T<6>, <7>: sweepO_inst.hip with -DCSIM_INST_WIDE)
template <int T>
hipError_t sweepO_wide_T(const double* in, double* out, int pitch, const Phys& p, const SweepCfg& cfg, const Bc2& bc,
                         const FinLines& fin, const SweepPlan& plan, hipStream_t st, const FrameSync& fs, const unsigned* lease);

// -------------------------------------------------------------------------------------------
// VAR_DPP — the default fused sweep.
// One wavefront owns a strip of 128 interior columns (2 per lane, one 16-byte load per lane
// per row = 8 full 128-byte lines per wave) and marches up `ry` rows keeping rows j-1, j, j+1
// of its own columns in registers, with PF further rows already in flight.  W/E neighbours
// come from the adjacent lanes by DPP; only lane 0 / lane 63 fetch the one column outside the
// strip (an L1/L2 hit: the neighbouring wave streams that line at the same time).  No LDS, no
// barriers, ~40 VGPRs -> 8 waves/SIMD.  HBM traffic per cell: 8 B read (+2/ry halo rows) + 8 B
// written.
// -------------------------------------------------------------------------------------------
template <int DIV, int PF>
__global__ __launch_bounds__(256) void k_sweep_dpp(const double* __restrict__ in,
                                                   double* __restrict__ out, int nx, int ny,
                                                   int pitch, int ry, int nwgx, int swz, Phys p) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lin = xcd_remap(blockIdx.x, gridDim.x, swz);
    const int wgx = lin % nwgx, chunk = lin / nwgx;
    const int c0 = (wgx * 4 + wave) * WAVE_COLS;
    if (c0 >= nx) return;  // wave-uniform
    const int jb = chunk * ry + 1;
    const int je = min(jb + ry - 1, ny);
    const int col = c0 + 2 * lane;
    const int nvalid = nx - col;
    const size_t xoff = static_cast<size_t>(LPAD + col);
    const bool edge_lane = (lane == 0) || (lane == 63);
    const size_t eoff = static_cast<size_t>(LPAD + c0 + (lane == 0 ? -1 : WAVE_COLS));

    auto ld2 = [&](int j) {
        return *reinterpret_cast<const double2*>(in + static_cast<size_t>(j) * pitch + xoff);
    };
    auto lde = [&](int j) {
        double e = 0.0;
        if (edge_lane) e = in[static_cast<size_t>(j) * pitch + eoff];
        return e;
    };

    double2 S = ld2(jb - 1);
    double2 C = ld2(jb);
    double eC = lde(jb);
    double2 q[PF];
    double eq[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        q[u] = make_double2(0.0, 0.0);
        eq[u] = 0.0;
        const int r = jb + 1 + u;
        if (r <= je + 1) {
            q[u] = ld2(r);
            eq[u] = lde(r);
        }
    }
    for (int j = jb; j <= je; j += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int jj = j + u;
            if (jj <= je) {  // wave-uniform
                const double2 N = q[u];
                const double eN = eq[u];
                const int r = jj + 1 + PF;
                if (r <= je + 1) {
                    q[u] = ld2(r);
                    eq[u] = lde(r);
                }
                const double Wx = from_prev_lane(C.y, eC);
                const double Ey = from_next_lane(C.x, eC);
                const double ox = cell<DIV>(C.x, Wx, C.y, S.x, N.x, p);
                const double oy = cell<DIV>(C.y, C.x, Ey, S.y, N.y, p);
                store_pair(out + static_cast<size_t>(jj) * pitch + xoff, ox, oy, nvalid);
                S = C;
                C = N;
                eC = eN;
            }
        }
    }
}

// -------------------------------------------------------------------------------------------
// VAR_LDS — LDS-staged marching sweep.  A 256-thread workgroup owns a 512-column strip; every
// row is loaded once (16 B per lane), staged in a double-buffered LDS row (ds_write_b128) with
// its two halo columns, and the W/E neighbours are read back from LDS (ds_read_b64); N/S stay
// in registers.  One workgroup barrier per row.
// LDS row layout (doubles): [1] = left halo, [2 .. 513] = strip, [514] = right halo.
// -------------------------------------------------------------------------------------------
constexpr int LDS_STRIP = 512;
template <int DIV>
__global__ __launch_bounds__(256) void k_sweep_lds(const double* __restrict__ in,
                                                   double* __restrict__ out, int nx, int ny,
                                                   int pitch, int ry, int nwgx, int swz, Phys p) {
    __shared__ __attribute__((aligned(16))) double rows[2][LDS_STRIP + 8];
    const int tid = threadIdx.x;
    const int lin = xcd_remap(blockIdx.x, gridDim.x, swz);
    const int wgx = lin % nwgx, chunk = lin / nwgx;
    const int c0 = wgx * LDS_STRIP;
    const int jb = chunk * ry + 1;
    const int je = min(jb + ry - 1, ny);
    const int col = c0 + 2 * tid;
    const int nvalid = nx - col;
    const size_t xoff = static_cast<size_t>(LPAD + col);
    const bool have = (LPAD + col + 1) < pitch;
    const bool halo_lane = (tid == 0) || (tid == 255);
    const size_t hoff = static_cast<size_t>(tid == 0 ? LPAD + c0 - 1 : LPAD + min(c0 + LDS_STRIP, nx));
    const int hidx = tid == 0 ? 1 : LDS_STRIP + 2;

    auto ld2 = [&](int j) {
        double2 v = make_double2(0.0, 0.0);
        if (have) v = *reinterpret_cast<const double2*>(in + static_cast<size_t>(j) * pitch + xoff);
        return v;
    };
    auto ldh = [&](int j) {
        double e = 0.0;
        if (halo_lane) e = in[static_cast<size_t>(j) * pitch + hoff];
        return e;
    };

    double2 S = ld2(jb - 1);
    double2 C = ld2(jb);
    {
        const double h = ldh(jb);
        *reinterpret_cast<double2*>(&rows[jb & 1][2 + 2 * tid]) = C;
        if (halo_lane) rows[jb & 1][hidx] = h;
    }
    __syncthreads();
    for (int j = jb; j <= je; ++j) {
        const double2 N = ld2(j + 1);
        const double hN = ldh(j + 1);
        const double* cur = rows[j & 1];
        const double Wx = cur[1 + 2 * tid];
        const double Ey = cur[4 + 2 * tid];
        double* nxt = rows[(j + 1) & 1];
        *reinterpret_cast<double2*>(&nxt[2 + 2 * tid]) = N;
        if (halo_lane) nxt[hidx] = hN;
        const double ox = cell<DIV>(C.x, Wx, C.y, S.x, N.x, p);
        const double oy = cell<DIV>(C.y, C.x, Ey, S.y, N.y, p);
        store_pair(out + static_cast<size_t>(j) * pitch + xoff, ox, oy, nvalid);
        S = C;
        C = N;
        __syncthreads();
    }
}

// VAR_NAIVE — one thread per cell pair, all five points straight from global memory (cache
// reuse only).  Kept as the measured baseline the tuned variants are compared against.
template <int DIV>
__global__ __launch_bounds__(256) void k_sweep_naive(const double* __restrict__ in,
                                                     double* __restrict__ out, int nx, int ny,
                                                     int pitch, Phys p) {
    const int col = (blockIdx.x * 256 + threadIdx.x) * 2;
    const int j = blockIdx.y + 1;
    if (col >= nx) return;
    const size_t o = static_cast<size_t>(j) * pitch + LPAD + col;
    const double2 C = *reinterpret_cast<const double2*>(in + o);
    const double2 N = *reinterpret_cast<const double2*>(in + o + pitch);
    const double2 S = *reinterpret_cast<const double2*>(in + o - pitch);
    const double W = in[o - 1];
    const double E = in[o + 2];
    const double ox = cell<DIV>(C.x, W, C.y, S.x, N.x, p);
    const double oy = cell<DIV>(C.y, C.x, E, S.y, N.y, p);
    store_pair(out + o, ox, oy, nx - col);
}

// ---- operators at the reference's own granularity (not the hot path) ------------------------
// MODE 0: out = diffusion(u) on the interior (reference src/diffusion.cpp:9-16)
// MODE 1: out += advection(u)               (reference src/advection.cpp:13-33)
template <int DIV, int MODE>
__global__ __launch_bounds__(256) void k_unit_op(const double* __restrict__ in,
                                                 double* __restrict__ out, int nx, int ny,
                                                 int pitch, Phys p) {
    const int i = blockIdx.x * 256 + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    if (i > nx) return;
    const size_t o = static_cast<size_t>(j) * pitch + (LPAD - 1) + i;
    const double c = in[o], W = in[o - 1], E = in[o + 1], S = in[o - pitch], N = in[o + pitch];
    if (MODE == 0)
        out[o] = diffuse_term<DIV>(c, W, E, S, N, p);
    else
        out[o] = out[o] + advect_term<DIV>(c, W, E, S, N, p);
}

// outer ring of `in` copied to `out` (reference src/diffusion.cpp:18-25)
__global__ void k_ring_copy(const double* __restrict__ in, double* __restrict__ out, int nx, int ny,
                            int pitch) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int nxt = nx + 2, nyt = ny + 2;
    if (t < nxt) {
        const size_t a = static_cast<size_t>(LPAD - 1 + t);
        out[a] = in[a];
        const size_t b = static_cast<size_t>(nyt - 1) * pitch + a;
        out[b] = in[b];
    }
    if (t < nyt) {
        const size_t a = static_cast<size_t>(t) * pitch + (LPAD - 1);
        out[a] = in[a];
        out[a + nxt - 1] = in[a + nxt - 1];
    }
}

__global__ void k_fill(double* __restrict__ f, int nx, int ny, int pitch, double v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i < nx + 2) f[static_cast<size_t>(j) * pitch + (LPAD - 1) + i] = v;
}

// apply_boundary on the HALO part of a physical side: where a Dirichlet/Neumann edge meets a
// neighbour side, the ghost line continues over the H halo cells that came from that neighbour
// (globally, they are the neighbour's own ghost cells of the same physical edge).  t = 8
// segments x H cells.  Inputs are halo cells written by the preceding k_halo2_unpack launch.
__device__ __forceinline__ void ghost_extend_cell(double* __restrict__ f, int nx, int ny, int pitch, int H,
                                                  const int bc[4], const int phys[4], double value, int t) {
    const int seg = t / H, k = t % H;
    if (seg >= 8) return;
    auto at2 = [&](int i, int j) -> double& { return f[static_cast<ptrdiff_t>(j) * pitch + (LPAD - 1) + i]; };
    // segments 0..3: physical bottom/top row over the left/right halo columns
    // segments 4..7: physical left/right column over the bottom/top halo rows
    if (seg < 4) {
        const int row_side = (seg & 1) ? CSIM_TOP : CSIM_BOTTOM, col_side = (seg & 2) ? CSIM_RIGHT : CSIM_LEFT;
        if (!phys[row_side] || phys[col_side] || bc[row_side] == CSIM_BC_PERIODIC) return;
        const int i = col_side == CSIM_LEFT ? -k : nx + 1 + k;
        const int jg = row_side == CSIM_BOTTOM ? 0 : ny + 1, ja = row_side == CSIM_BOTTOM ? 1 : ny;
        at2(i, jg) = bc[row_side] == CSIM_BC_DIRICHLET ? value : at2(i, ja);
    } else {
        const int col_side = (seg & 1) ? CSIM_RIGHT : CSIM_LEFT, row_side = (seg & 2) ? CSIM_TOP : CSIM_BOTTOM;
        if (!phys[col_side] || phys[row_side] || bc[col_side] == CSIM_BC_PERIODIC) return;
        const int j = row_side == CSIM_BOTTOM ? -k : ny + 1 + k;
        const int ig = col_side == CSIM_LEFT ? 0 : nx + 1, ia = col_side == CSIM_LEFT ? 1 : nx;
        at2(ig, j) = bc[col_side] == CSIM_BC_DIRICHLET ? value : at2(ia, j);
    }
}

__global__ __launch_bounds__(256) void k_ghost_fill(double* __restrict__ a, double* __restrict__ b,
                                                    int nx, int ny, int pitch, GhostDev g) {
    __builtin_amdgcn_s_setprio(3);  // short latency-critical kernel, usually sharing the SIMDs with a bulk sweep
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int tc = nx > ny ? nx : ny;
    if (g.ext_depth > 0 && t > tc && t <= tc + 8 * g.ext_depth) {
        // (same values as the corner thread wherever the two overlap, so the order is immaterial)
        ghost_extend_cell(a, nx, ny, pitch, g.ext_depth, g.bc, g.phys, g.value, t - tc - 1);
        return;
    }
    ghost_fill_cell(a, b, nx, ny, pitch, g, t);
}

// The four edge lines of the NEXT field, computed from the current one and written directly
// into the send staging buffers, so the RCCL exchange can start before (and overlap with) the
// full sweep.  Same arithmetic as the sweep => the values sent equal the values later stored.
template <int DIV>
__global__ __launch_bounds__(256) void k_edge_pack(const double* __restrict__ in, int nx, int ny,
                                                   int pitch, Phys p, double* sl, double* sr,
                                                   double* sb, double* st) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    auto upd = [&](int i, int j) {
        const size_t o = at(i, j, pitch);
        return cell<DIV>(in[o], in[o - 1], in[o + 1], in[o - pitch], in[o + pitch], p);
    };
    if (t < ny) {
        if (sl) sl[t] = upd(1, t + 1);
        if (sr) sr[t] = upd(nx, t + 1);
    }
    if (t < nx) {
        if (sb) sb[t] = upd(t + 1, 1);
        if (st) st[t] = upd(t + 1, ny);
    }
}

__global__ __launch_bounds__(256) void k_pack(const double* __restrict__ in, int nx, int ny, int pitch,
                                              double* sl, double* sr, double* sb, double* st) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < ny) {
        if (sl) sl[t] = in[at(1, t + 1, pitch)];
        if (sr) sr[t] = in[at(nx, t + 1, pitch)];
    }
    if (t < nx) {
        if (sb) sb[t] = in[at(t + 1, 1, pitch)];
        if (st) st[t] = in[at(t + 1, ny, pitch)];
    }
}

// ---- deep faces for the multi-step sweep on several ranks (depth H = 2..7) --------------------
// Directions: 0 left, 1 right, 2 bottom, 3 top, 4 bottom-left, 5 bottom-right, 6 top-left,
// 7 top-right.  Faces hold the H outermost interior columns (H x (ny+2)), rows (H x (nx+2); ghost
// entries included so Periodic ghosts travel with them) or the H x H corner block.
struct Halo2Ptrs {
    double* p[8];
};

// H = face depth (= time steps of the fused pass that will consume the faces, 2..7).
// Column faces span rows 0..ny+1 and row faces columns 0..nx+1, i.e. they carry the sender's
// ghost entries along, so that Periodic (never rewritten) ghosts reach the neighbour.
__global__ __launch_bounds__(256) void k_halo2_pack(const double* __restrict__ f, int nx, int ny,
                                                    int pitch, int H, Halo2Ptrs s) {
    __builtin_amdgcn_s_setprio(3);  // short latency-critical kernel, usually sharing the SIMDs with a bulk sweep
    const int t = blockIdx.x * 256 + threadIdx.x;
    auto ld = [&](int i, int j) { return f[static_cast<ptrdiff_t>(j) * pitch + (LPAD - 1) + i]; };
    if (t < H * (ny + 2)) {
        const int c = t / (ny + 2), j = t % (ny + 2);
        if (s.p[0]) s.p[0][t] = ld(1 + c, j);
        if (s.p[1]) s.p[1][t] = ld(nx - H + 1 + c, j);
    }
    if (t < H * (nx + 2)) {
        const int r = t / (nx + 2), i = t % (nx + 2);
        if (s.p[2]) s.p[2][t] = ld(i, 1 + r);
        if (s.p[3]) s.p[3][t] = ld(i, ny - H + 1 + r);
    }
    if (t < H * H) {
        const int r = t / H, c = t % H;
        if (s.p[4]) s.p[4][t] = ld(1 + c, 1 + r);
        if (s.p[5]) s.p[5][t] = ld(nx - H + 1 + c, 1 + r);
        if (s.p[6]) s.p[6][t] = ld(1 + c, ny - H + 1 + r);
        if (s.p[7]) s.p[7][t] = ld(nx - H + 1 + c, ny - H + 1 + r);
    }
}

// r.p[d] = face received FROM direction d (the neighbour's face of the opposite direction).
// The ghost entries a face carries are kept only where the crossing side is a physical edge;
// next to a neighbour side the corner block of the diagonal rank supplies those cells.
__global__ __launch_bounds__(256) void k_halo2_unpack(double* __restrict__ f, int nx, int ny, int pitch,
                                                      int H, Halo2Ptrs r) {
    __builtin_amdgcn_s_setprio(3);  // short latency-critical kernel, usually sharing the SIMDs with a bulk sweep
    const int t = blockIdx.x * 256 + threadIdx.x;
    auto st = [&](int i, int j, double v) { f[static_cast<ptrdiff_t>(j) * pitch + (LPAD - 1) + i] = v; };
    if (t < H * (ny + 2)) {
        const int c = t / (ny + 2), j = t % (ny + 2);
        const bool keep = (j >= 1 && j <= ny) || (j == 0 && !r.p[2]) || (j == ny + 1 && !r.p[3]);
        if (keep) {
            if (r.p[0]) st(1 - H + c, j, r.p[0][t]);
            if (r.p[1]) st(nx + 1 + c, j, r.p[1][t]);
        }
    }
    if (t < H * (nx + 2)) {
        const int q = t / (nx + 2), i = t % (nx + 2);
        const bool keep = (i >= 1 && i <= nx) || (i == 0 && !r.p[0]) || (i == nx + 1 && !r.p[1]);
        if (keep) {
            if (r.p[2]) st(i, 1 - H + q, r.p[2][t]);
            if (r.p[3]) st(i, ny + 1 + q, r.p[3][t]);
        }
    }
    if (t < H * H) {
        const int q = t / H, c = t % H;
        if (r.p[4]) st(1 - H + c, 1 - H + q, r.p[4][t]);
        if (r.p[5]) st(nx + 1 + c, 1 - H + q, r.p[5][t]);
        if (r.p[6]) st(1 - H + c, ny + 1 + q, r.p[6][t]);
        if (r.p[7]) st(nx + 1 + c, ny + 1 + q, r.p[7][t]);
    }
}

// gaussian hotspot on the device (reference src/init.cpp:12-33); exp() may differ from glibc
// in the last ulp, so parity runs upload a host-made field instead.
__global__ __launch_bounds__(256) void k_gaussian(double* __restrict__ f, int nx, int ny, int pitch,
                                                  int x_off, int y_off, double dx, double dy,
                                                  double A, double xc, double yc, double sig) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= nx) return;
    const double x = (x_off + i + 0.5) * dx;
    const double y = (y_off + j + 0.5) * dy;
    const double r2 = (x - xc) * (x - xc) + (y - yc) * (y - yc);
    f[at(i + 1, j + 1, pitch)] = A * exp(-r2 / (2.0 * sig * sig));
}

// ---- reductions: Field, Stepper (gridDim.y == 1, slab == 0) and ensemble (blockIdx.y = member, slab = its stride) ----
// KIND 0: min/max over i0..i1, j0..j1 ; KIND 1: sum ; KIND 2: max |a-b| ; KIND 3: the screen lease's verdict (below)
// Block b of a member takes rows j0 + b, j0 + b + G, ... (G = gridDim.x); its result goes to partial[m * G + b], the
// maximum of KIND 0 to partial[gridDim.y * G + m * G + b]; fold_partials (api.cpp) merges a member's blocks in order.
// NaN: min/max skip it (fmin / fmax; all NaN gives +inf, -inf), the sum carries it, and max |a-b| is NaN as soon as
// one |a-b| is — max_nan (internal.hpp) at all of its stages, and again on the host (fold_partials), where fmax would lose it.
// The sum's order is fixed (tests/reduce_restatement.py restates it): a lane adds its columns of its rows serially,
// then the xor butterfly of wave_sum, the four waves in order, the blocks in order on the host.
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double wave_max_nan(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max_nan(v, __shfl_xor(v, m, 64));
    return v;
}
// KIND 3 (launch_lease; gridDim.y == 1): the window is the whole field with its ring, i0 = j0 = 0, i1 = nx + 1,
// j1 = ny + 1, and a cell on the window's rim is a ring cell.  r0 / r1 are min / max of |v| over the non-zero finite
// values, and a third partial carries the flags LF_* (as a small integer in a double).  Each block adds itself to a
// ticket after its partials are out (release fence, agent scope); the block that draws the last ticket folds all
// partials (read past the caches) and stores the verdict — the host never reads it on the step path.
enum : unsigned {
    LF_POS = 1, LF_NEG = 2,            // an interior value > 0 / < 0
    LF_ZERO = 4,                       // an interior value that is a zero of either sign
    LF_RING_POS = 8, LF_RING_NEG = 16, // a ring value > 0 / < 0
    LF_RING_PZ = 32, LF_RING_NZ = 64,  // a ring value that is +0 / -0
    LF_NONFINITE = 128                 // any value that is Inf or NaN
};
struct LeaseOut {
    double M_req = 0.0, m_req = 0.0;
    unsigned* word = nullptr;  // word[0]: the verdict, word[1]: the ticket counter
};
__device__ __forceinline__ unsigned lease_verdict(double lo, double hi, unsigned f, const LeaseOut& q) {
    const bool upper = q.M_req > 0.0 && !(f & LF_NONFINITE) && hi <= q.M_req;
    // one sign throughout: the interior strictly, the ring with zeros of that sign allowed
    const bool pos = !(f & (LF_NEG | LF_RING_NEG | LF_RING_NZ)) && (f & LF_POS);
    const bool neg = !(f & (LF_POS | LF_RING_POS | LF_RING_PZ)) && (f & LF_NEG);
    const bool lower = q.m_req > 0.0 && !(f & LF_ZERO) && (pos || neg) && lo >= q.m_req;
    return (upper ? 1u : 0u) | (upper && lower ? 2u : 0u);
}

template <int KIND>
__global__ __launch_bounds__(256) void k_reduce(const double* __restrict__ a,
                                                const double* __restrict__ b, int i0, int i1,
                                                int j0, int j1, int pitch, long slab,
                                                double* __restrict__ partial, LeaseOut lease) {
    __shared__ double sh[2][4];
    __shared__ unsigned shf[4];
    a += static_cast<ptrdiff_t>(blockIdx.y) * slab;
    if (KIND == 2) b += static_cast<ptrdiff_t>(blockIdx.y) * slab;
    double r0 = (KIND == 0 || KIND == 3) ? INFINITY : 0.0;  // min | sum | linf | min |v|
    double r1 = KIND == 3 ? 0.0 : -INFINITY;                // max | max |v|
    unsigned fl = 0;
    if (KIND == 3) {
        // A row's interior starts on a 128-byte boundary at column 1 (internal.hpp): the lanes take it as double2 pairs,
        // eight in flight each (the launch is one read of the field and should run at HBM speed); thread 0 adds the two
        // ring columns and the last column of an odd width.
        auto take = [&](double v, bool ring) {
            const double m = fabs(v);
            if (!(m < INFINITY)) {  // Inf or NaN
                fl |= LF_NONFINITE;
            } else if (m == 0.0) {
                fl |= ring ? (signbit(v) ? LF_RING_NZ : LF_RING_PZ) : LF_ZERO;
            } else {
                fl |= ring ? (v > 0.0 ? LF_RING_POS : LF_RING_NEG) : (v > 0.0 ? LF_POS : LF_NEG);
                r0 = fmin(r0, m);
                r1 = fmax(r1, m);
            }
        };
        const int nx = i1 - i0 - 1, npair = nx >> 1;
        for (int j = j0 + blockIdx.x; j <= j1; j += gridDim.x) {
            const bool ring_row = j == j0 || j == j1;
            const double* row = a + at(i0 + 1, j, pitch);
#pragma unroll 8
            for (int k = threadIdx.x; k < npair; k += 256) {
                const double2 v = *reinterpret_cast<const double2*>(row + 2 * k);
                take(v.x, ring_row);
                take(v.y, ring_row);
            }
            if (threadIdx.x == 0) {
                take(row[-1], true);
                take(row[nx], true);
                if (nx & 1) take(row[nx - 1], ring_row);
            }
        }
    }
    for (int j = j0 + blockIdx.x; KIND != 3 && j <= j1; j += gridDim.x) {
        for (int i = i0 + threadIdx.x; i <= i1; i += 256) {
            const size_t o = at(i, j, pitch);
            const double v = a[o];
            if (KIND == 0) {
                r0 = fmin(r0, v);
                r1 = fmax(r1, v);
            } else if (KIND == 1) {
                r0 = r0 + v;
            } else {
                r0 = max_nan(r0, fabs(v - b[o]));
            }
        }
    }
    if (KIND == 0 || KIND == 3) {
        r0 = wave_min(r0);
        r1 = wave_max(r1);
        if (KIND == 3) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) fl |= __shfl_xor(fl, m, 64);
        }
    } else if (KIND == 1) {
        r0 = wave_sum(r0);
    } else {
        r0 = wave_max_nan(r0);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sh[0][wave] = r0;
        sh[1][wave] = r1;
        shf[wave] = fl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double x0 = sh[0][0], x1 = sh[1][0];
        for (int w = 1; w < 4; ++w) {
            if (KIND == 0 || KIND == 3) {
                x0 = fmin(x0, sh[0][w]);
                x1 = fmax(x1, sh[1][w]);
            } else if (KIND == 1) {
                x0 = x0 + sh[0][w];
            } else {
                x0 = max_nan(x0, sh[0][w]);
            }
        }
        const size_t k = static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x;
        partial[k] = x0;
        if (KIND == 0 || KIND == 3) partial[static_cast<size_t>(gridDim.y) * gridDim.x + k] = x1;
        if (KIND == 3) partial[2 * static_cast<size_t>(gridDim.x) + k] = static_cast<double>(shf[0] | shf[1] | shf[2] | shf[3]);
    }
    if (KIND == 3) {
        // the last block to arrive folds: its wave 0 reads every block's three partials (agent-scope loads, past this
        // XCD's caches; the writers' fences came before their tickets) and one lane stores the verdict
        __shared__ bool is_last;
        if (threadIdx.x == 0) {
            __threadfence();
            is_last = atomicAdd(lease.word + 1, 1u) == gridDim.x - 1;
        }
        __syncthreads();
        if (is_last && wave == 0) {
            __threadfence();
            const int G = gridDim.x;
            auto ld = [&](int idx) {
                return __longlong_as_double(static_cast<long long>(__hip_atomic_load(
                    reinterpret_cast<const unsigned long long*>(partial + idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
            };
            double lo = INFINITY, hi = 0.0;
            unsigned f = 0;
            for (int k = lane; k < G; k += 64) {
                lo = fmin(lo, ld(k));
                hi = fmax(hi, ld(G + k));
                f |= static_cast<unsigned>(ld(2 * G + k));
            }
            lo = wave_min(lo);
            hi = wave_max(hi);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) f |= __shfl_xor(f, m, 64);
            if (lane == 0) {
                lease.word[0] = lease_verdict(lo, hi, f, lease);
                lease.word[1] = 0u;  // the ticket counter, for the next launch
            }
        }
    }
}

// Position-weighted 64-bit checksum of the interior: sum over cells of bits(u) * (K + 2 g) mod 2^64, g = the cell's
// GLOBAL linear index.  Every multiplier is odd, so any change of any cell changes the sum, and because the
// weights follow the global position the per-rank sums of a decomposed field add up (mod 2^64) to the checksum
// of the same field held by one rank — the bit-identity check a multi-GPU run can carry in one number.
// Members as in k_reduce; an ensemble's members are whole fields: x_off = y_off = 0, nx_global = nx.
__global__ __launch_bounds__(256) void k_checksum(const double* __restrict__ f, int nx, int ny, int pitch, long slab,
                                                  long x_off, long y_off, long nx_global,
                                                  unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long sh[4];
    f += static_cast<ptrdiff_t>(blockIdx.y) * slab;
    unsigned long long acc = 0;
    for (int j = 1 + blockIdx.x; j <= ny; j += gridDim.x) {
        const unsigned long long row = static_cast<unsigned long long>(y_off + j - 1) * static_cast<unsigned long long>(nx_global) +
                                       static_cast<unsigned long long>(x_off);
        for (int i = 1 + threadIdx.x; i <= nx; i += 256) {
            const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(f[at(i, j, pitch)]));
            acc += bits * (0x9E3779B97F4A7C15ull + 2ull * (row + static_cast<unsigned long long>(i - 1)));
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// ============================================================================================
// launchers
// ============================================================================================

template <int DIV>
static hipError_t sweep_div(const double* in, double* out, int nx, int ny, int pitch, const Phys& p,
                            const SweepCfg& cfg, hipStream_t st) {
    int variant = cfg.variant == VAR_AUTO ? VAR_DPP : cfg.variant;
    int ry = cfg.rows_per_chunk > 0 ? cfg.rows_per_chunk : 64;
    if (ry > ny) ry = ny;
    const int nchunks = cdiv(ny, ry);
    if (variant == VAR_NAIVE) {
        dim3 grid(cdiv(nx, 512), ny);
        hipLaunchKernelGGL(k_sweep_naive<DIV>, grid, dim3(256), 0, st, in, out, nx, ny, pitch, p);
    } else if (variant == VAR_LDS) {
        const int nwgx = cdiv(nx, LDS_STRIP);
        hipLaunchKernelGGL(k_sweep_lds<DIV>, dim3(nwgx * nchunks), dim3(256), 0, st, in, out, nx, ny,
                           pitch, ry, nwgx, cfg.xcd_swizzle, p);
    } else {
        const int nwgx = cdiv(cdiv(nx, WAVE_COLS), 4);
        const dim3 grid(nwgx * nchunks);
        const int pf = cfg.prefetch > 0 ? cfg.prefetch : 2;
        if (pf <= 1)
            hipLaunchKernelGGL((k_sweep_dpp<DIV, 1>), grid, dim3(256), 0, st, in, out, nx, ny, pitch,
                               ry, nwgx, cfg.xcd_swizzle, p);
        else if (pf == 2)
            hipLaunchKernelGGL((k_sweep_dpp<DIV, 2>), grid, dim3(256), 0, st, in, out, nx, ny, pitch,
                               ry, nwgx, cfg.xcd_swizzle, p);
        else if (pf <= 4)
            hipLaunchKernelGGL((k_sweep_dpp<DIV, 4>), grid, dim3(256), 0, st, in, out, nx, ny, pitch,
                               ry, nwgx, cfg.xcd_swizzle, p);
        else
            hipLaunchKernelGGL((k_sweep_dpp<DIV, 8>), grid, dim3(256), 0, st, in, out, nx, ny, pitch,
                               ry, nwgx, cfg.xcd_swizzle, p);
    }
    return hipGetLastError();
}

// overlapped-strip multi-step sweep, T = 2..7 (kind[] / part: see internal.hpp)
hipError_t launch_sweepO(const double* in, double* out, int pitch, const Phys& p, const SweepCfg& cfg,
                         const int kind[4], double value, const SweepPlan& plan, hipStream_t st,
                         double* const fin_lines[4], const FrameSync* sync, const unsigned* lease) {
    Bc2 bc;
    for (int s = 0; s < 4; ++s) bc.kind[s] = kind[s];
    bc.value = value;
    FinLines fin;
    for (int s = 0; s < 4; ++s) fin.line[s] = fin_lines ? fin_lines[s] : nullptr;
    const FrameSync fs = sync ? *sync : FrameSync{};
    if (plan.wide) {  // a missing instantiation is an error, not another kernel
        if (plan.T == 6) return sweepO_wide_T<6>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
        if (plan.T == 7) return sweepO_wide_T<7>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
        return hipErrorInvalidValue;
    }
    switch (plan.T) {
        case 2: return sweepO_T<2>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
        case 3: return sweepO_T<3>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
        case 4: return sweepO_T<4>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
        case 5: return sweepO_T<5>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
        case 6: return sweepO_T<6>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
        default: return sweepO_T<7>(in, out, pitch, p, cfg, bc, fin, plan, st, fs, lease);
    }
}

hipError_t launch_halo2_pack(const double* f, int nx, int ny, int pitch, int depth,
                             double* const send[8], hipStream_t st) {
    Halo2Ptrs s;
    for (int d = 0; d < 8; ++d) s.p[d] = send[d];
    const int n = depth * (std::max(ny, nx) + 2);
    hipLaunchKernelGGL(k_halo2_pack, dim3(cdiv(n, 256)), dim3(256), 0, st, f, nx, ny, pitch, depth, s);
    return hipGetLastError();
}

hipError_t launch_halo2_unpack(double* f, int nx, int ny, int pitch, int depth,
                               double* const recv[8], hipStream_t st) {
    Halo2Ptrs r;
    for (int d = 0; d < 8; ++d) r.p[d] = recv[d];
    const int n = depth * (std::max(ny, nx) + 2);
    hipLaunchKernelGGL(k_halo2_unpack, dim3(cdiv(n, 256)), dim3(256), 0, st, f, nx, ny, pitch, depth, r);
    return hipGetLastError();
}

hipError_t launch_sweep(const double* in, double* out, int nx, int ny, int pitch, const Phys& p,
                        const SweepCfg& cfg, hipStream_t st) {
    switch (p.div_mode) {
        case 0: return sweep_div<0>(in, out, nx, ny, pitch, p, cfg, st);
        case 1: return sweep_div<1>(in, out, nx, ny, pitch, p, cfg, st);
        case 3: return sweep_div<3>(in, out, nx, ny, pitch, p, cfg, st);
        default: return sweep_div<2>(in, out, nx, ny, pitch, p, cfg, st);
    }
}

template <int MODE>
static hipError_t unit_op(const double* in, double* out, int nx, int ny, int pitch, const Phys& p,
                          hipStream_t st) {
    dim3 grid(cdiv(nx, 256), ny);
    switch (p.div_mode) {
        case 0: hipLaunchKernelGGL((k_unit_op<0, MODE>), grid, dim3(256), 0, st, in, out, nx, ny, pitch, p); break;
        case 1: hipLaunchKernelGGL((k_unit_op<1, MODE>), grid, dim3(256), 0, st, in, out, nx, ny, pitch, p); break;
        default: hipLaunchKernelGGL((k_unit_op<2, MODE>), grid, dim3(256), 0, st, in, out, nx, ny, pitch, p); break;
    }
    return hipGetLastError();
}

hipError_t launch_diffusion_only(const double* in, double* out, int nx, int ny, int pitch,
                                 const Phys& p, hipStream_t st) {
    return unit_op<0>(in, out, nx, ny, pitch, p, st);
}
hipError_t launch_advection_only(const double* in, double* out, int nx, int ny, int pitch,
                                 const Phys& p, hipStream_t st) {
    return unit_op<1>(in, out, nx, ny, pitch, p, st);
}

hipError_t launch_ring_copy(const double* in, double* out, int nx, int ny, int pitch, hipStream_t st) {
    const int n = (nx > ny ? nx : ny) + 2;
    hipLaunchKernelGGL(k_ring_copy, dim3(cdiv(n, 256)), dim3(256), 0, st, in, out, nx, ny, pitch);
    return hipGetLastError();
}

hipError_t launch_fill(double* f, int nx, int ny, int pitch, double v, hipStream_t st) {
    hipLaunchKernelGGL(k_fill, dim3(cdiv(nx + 2, 256), ny + 2), dim3(256), 0, st, f, nx, ny, pitch, v);
    return hipGetLastError();
}

hipError_t launch_ghost_fill(double* a, double* b, int nx, int ny, int pitch, const GhostArgs& g,
                             hipStream_t st, int ext_depth) {
    GhostDev d;
    d.ext_depth = ext_depth;
    for (int s = 0; s < 4; ++s) {
        d.bc[s] = g.bc[s];
        d.phys[s] = g.phys[s];
        d.recv[s] = g.recv[s];
        d.adj[s] = g.adj[s];
    }
    d.value = g.value;
    const int n = (nx > ny ? nx : ny) + 1 + 8 * ext_depth;
    hipLaunchKernelGGL(k_ghost_fill, dim3(cdiv(n, 256)), dim3(256), 0, st, a, b, nx, ny, pitch, d);
    return hipGetLastError();
}

hipError_t launch_edge_pack(const double* in, int nx, int ny, int pitch, const Phys& p,
                            double* const send[4], hipStream_t st) {
    const int n = nx > ny ? nx : ny;
    const dim3 grid(cdiv(n, 256));
    switch (p.div_mode) {
        case 0: hipLaunchKernelGGL(k_edge_pack<0>, grid, dim3(256), 0, st, in, nx, ny, pitch, p, send[0], send[1], send[2], send[3]); break;
        case 1: hipLaunchKernelGGL(k_edge_pack<1>, grid, dim3(256), 0, st, in, nx, ny, pitch, p, send[0], send[1], send[2], send[3]); break;
        case 3: hipLaunchKernelGGL(k_edge_pack<3>, grid, dim3(256), 0, st, in, nx, ny, pitch, p, send[0], send[1], send[2], send[3]); break;
        default: hipLaunchKernelGGL(k_edge_pack<2>, grid, dim3(256), 0, st, in, nx, ny, pitch, p, send[0], send[1], send[2], send[3]); break;
    }
    return hipGetLastError();
}

hipError_t launch_pack(const double* in, int nx, int ny, int pitch, double* const send[4],
                       hipStream_t st) {
    const int n = nx > ny ? nx : ny;
    hipLaunchKernelGGL(k_pack, dim3(cdiv(n, 256)), dim3(256), 0, st, in, nx, ny, pitch, send[0],
                       send[1], send[2], send[3]);
    return hipGetLastError();
}

hipError_t launch_gaussian(double* f, int nx, int ny, int pitch, int x_off, int y_off, int nxg,
                           int nyg, double dx, double dy, double A, double sigma_frac,
                           double xc_frac, double yc_frac, hipStream_t st) {
    const double Lx = nxg * dx, Ly = nyg * dy;
    const double xc = xc_frac * Lx, yc = yc_frac * Ly;
    const double sig = sigma_frac * (Lx < Ly ? Lx : Ly);
    hipLaunchKernelGGL(k_gaussian, dim3(cdiv(nx, 256), ny), dim3(256), 0, st, f, nx, ny, pitch, x_off,
                       y_off, dx, dy, A, xc, yc, sig);
    return hipGetLastError();
}

hipError_t launch_minmax(const double* f, int nx, int ny, int pitch, double* scratch, hipStream_t st, const Members& mb) {
    hipLaunchKernelGGL(k_reduce<0>, dim3(reduce_blocks(ny + 2, mb.cap), mb.count), dim3(256), 0, st, f, nullptr, 0,
                       nx + 1, 0, ny + 1, pitch, mb.slab, scratch, LeaseOut{});
    return hipGetLastError();
}
hipError_t launch_sum(const double* f, int nx, int ny, int pitch, double* scratch, hipStream_t st, const Members& mb) {
    hipLaunchKernelGGL(k_reduce<1>, dim3(reduce_blocks(ny, mb.cap), mb.count), dim3(256), 0, st, f, nullptr, 1, nx, 1,
                       ny, pitch, mb.slab, scratch, LeaseOut{});
    return hipGetLastError();
}
hipError_t launch_linf(const double* a, const double* b, int nx, int ny, int pitch, double* scratch,
                       hipStream_t st) {
    hipLaunchKernelGGL(k_reduce<2>, dim3(reduce_blocks(ny, REDUCE_BLOCKS)), dim3(256), 0, st, a, b, 1, nx, 1, ny, pitch,
                       0L, scratch, LeaseOut{});
    return hipGetLastError();
}

hipError_t launch_lease(const double* f, int nx, int ny, int pitch, double* scratch, double M_req, double m_req,
                        unsigned* lease, hipStream_t st) {
    LeaseOut q;
    q.M_req = M_req, q.m_req = m_req, q.word = lease;
    hipLaunchKernelGGL(k_reduce<3>, dim3(reduce_blocks(ny + 2, LEASE_BLOCKS)), dim3(256), 0, st, f, nullptr, 0, nx + 1, 0,
                       ny + 1, pitch, 0L, scratch, q);
    return hipGetLastError();
}

hipError_t launch_checksum(const double* f, int nx, int ny, int pitch, long x_off, long y_off, long nx_global,
                           double* scratch, hipStream_t st, const Members& mb) {
    hipLaunchKernelGGL(k_checksum, dim3(reduce_blocks(ny, mb.cap), mb.count), dim3(256), 0, st, f, nx, ny, pitch, mb.slab,
                       x_off, y_off, nx_global, reinterpret_cast<unsigned long long*>(scratch));
    return hipGetLastError();
}

}  // namespace csim
