// api.cpp — the C ABI of include/csim.h, part 1: library / device, host-side scalars, MPI-free decomposition,
// the exchange plan, the device Field mirror and the reference-granularity operators.  (The time-loop stepper:
// stepper.cpp, passes.cpp, planner.cpp, profile.cpp; kernels: kernels.hip, sweepO.hpp, sweep_core.hpp.)  Compiled with hipcc; host code only.
#include "stepper.hpp"

namespace csim {

static thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
static bool pow2(double x) {
    if (!(x > 0.0) || !std::isnormal(x)) return false;
    int e = 0;
    return std::frexp(x, &e) == 0.5 && std::isnormal(1.0 / x);
}

// g, the bound on the growth of max|u| per step: the sum of the magnitudes of what multiplies the five points, with
// room for the 15 roundings (make_phys: fast_thr; lease_bounds: M_req)
static double growth_per_step(const Phys& p) {
    return (1.0 + 4.0 * std::fabs(p.kdiff) * (1.0 / p.dx2 + 1.0 / p.dy2) +
            2.0 * std::fabs(p.mdt) * (std::fabs(p.vx) / std::fabs(p.dx) + std::fabs(p.vy) / std::fabs(p.dy))) * (1.0 + 1e-9);
}

// The screen lease's bounds (internal.hpp; derivation: DESIGN.md §4), in exponents like slow_thr above so that nothing
// under- or overflows on the way: both come out as powers of two, M_req rounded down and m_req rounded up by a whole
// binade more than the logarithms' own error could ask for.
//   upper: max|u| grows by at most g per step whatever the signs, so max|u| <= U / g^(R + MAX_FUSE) now keeps every
//     value a pass loads within R steps below U = p2_hi (fast_thr where the 12-operation form is off) — and the
//     thresholds themselves carry the levels inside a pass.
//   lower: with a0, aW, aE, aS, aN > 0 and a field of one sign (ring zeros allowed) the exact update of a cell is at
//     least a0 c and at least a_min max_local.  Each of the at most 15 roundings of either form is relative to an
//     intermediate that, carried through the factors still to come, is at most g max_local, so
//     |computed - exact| <= 16 g eps max_local <= (16 g eps / a_min) exact; eta doubles that for the rounding of the
//     coefficients themselves.  Hence min|u| shrinks by at most a0 (1 - eta) per step, and min|u| >= 2 slow_thr /
//     (a0 (1 - eta))^(R + MAX_FUSE) now keeps every non-zero value a pass loads within R steps at or above 2 slow_thr.
//     (No bit is lost to the subnormal range on the way: that is slow_thr's own grid argument.)
LeaseBounds lease_bounds(const Phys& p, long R) {
    LeaseBounds b;
    if (R < 1 || p.div_mode > 1 || !(p.fast_thr > 0.0)) return b;
    const double g = growth_per_step(p);
    if (!std::isfinite(g) || !(g >= 1.0)) return b;
    const double n = static_cast<double>(R) + MAX_FUSE;
    const double upper = p.slow_thr > 0.0 ? p.p2_hi : p.fast_thr;
    const double eM = std::floor(std::log2(upper) - n * std::log2(g)) - 1.0;
    if (!(eM >= -1000.0)) return b;  // a lease this long leaves no field to admit
    b.M_req = std::ldexp(1.0, static_cast<int>(eM));
    const double coef[5] = {p.a0, p.aW, p.aE, p.aS, p.aN};
    double a_min = coef[0];
    for (double c : coef) a_min = (c > 0.0 && std::isfinite(c)) ? std::min(a_min, c) : 0.0;
    if (!(p.slow_thr > 0.0) || !(a_min > 0.0)) return b;
    const double eta = 32.0 * g * std::ldexp(1.0, -53) / a_min;
    if (!(eta <= std::ldexp(1.0, -20)) || !(p.a0 < 1.0)) return b;  // a coefficient so small that rounding could eat the bound
    const double em = std::ceil(std::log2(p.slow_thr) + 1.0 - n * (std::log2(p.a0) + std::log1p(-eta) / std::log(2.0))) + 1.0;
    if (!(em <= eM)) return b;  // no value could satisfy both
    b.m_req = std::ldexp(1.0, static_cast<int>(em));
    b.eta = eta;
    return b;
}

Phys make_phys(double dx, double dy, double D, double dt, double vx, double vy, bool contract) {
    Phys p;
    p.kdiff = dt * D;
    p.mdt = -dt;
    p.vx = vx;
    p.vy = vy;
    p.dx = dx;
    p.dy = dy;
    p.dx2 = dx * dx;
    p.dy2 = dy * dy;
    p.rdx = 1.0 / dx;
    p.rdy = 1.0 / dy;
    p.rdx2 = 1.0 / p.dx2;
    p.rdy2 = 1.0 / p.dy2;
    if (dx == 1.0 && dy == 1.0)
        p.div_mode = 0;
    else if (pow2(dx) && pow2(dy) && pow2(p.dx2) && pow2(p.dy2))
        p.div_mode = 1;
    else
        p.div_mode = 2;
    // coefficient form of the same update (option "contract"): collect what multiplies each of the five
    // points in  c + dt D ((E - 2c + W)/dx^2 + (N - 2c + S)/dy^2) - dt (vx dudx + vy dudy)  with the
    // upwind differences dudx = (c - W)/dx for vx >= 0, (E - c)/dx otherwise (dudy likewise)
    {
        const long double kx = static_cast<long double>(dt) * D / (static_cast<long double>(dx) * dx);
        const long double ky = static_cast<long double>(dt) * D / (static_cast<long double>(dy) * dy);
        const long double cx = static_cast<long double>(dt) * vx / dx, cy = static_cast<long double>(dt) * vy / dy;
        const long double acx = cx < 0 ? -cx : cx, acy = cy < 0 ? -cy : cy;
        p.a0 = static_cast<double>(1.0L - 2.0L * kx - 2.0L * ky - acx - acy);
        p.aW = static_cast<double>(kx + (vx >= 0.0 ? acx : 0.0L));
        p.aE = static_cast<double>(kx + (vx >= 0.0 ? 0.0L : acx));
        p.aS = static_cast<double>(ky + (vy >= 0.0 ? acy : 0.0L));
        p.aN = static_cast<double>(ky + (vy >= 0.0 ? 0.0L : acy));
    }
    // fused E - 2c (diffuse_term<., true>): max|u| grows by at most g per step — the sum of the magnitudes of
    // what multiplies the five points, with room for the 15 roundings — so a tile whose inputs stay below
    // 2^1022 / g^MAX_FUSE cannot reach 2^1023 at any level of a pass.  Parameters so far from stable that
    // this bound drops below 2^900 switch the fused form off.
    {
        const double g = growth_per_step(p);
        const double thr = std::ldexp(1.0, 1022) / std::pow(g, MAX_FUSE);
        p.fast_thr = (std::isfinite(g) && thr >= std::ldexp(1.0, 900)) ? thr : 0.0;
    }
    // Power-of-two velocities (cell<.., P2>; derivation: DESIGN.md §4).  A = vx/dx and B = vy/dy are signed powers of
    // two; the one factored out is vy unless only vx is positive.  Everything below is in exponents, so that no bound
    // under- or overflows while it is being formed.
    //   grid: every value a screened tile loads is 0 or >= L = 2^eL in magnitude, hence a multiple of G0 = 2^(eL - 52).
    //   Sums, differences and the exact fmas of multiples of G are multiples of G.  A product with a power of two 2^e
    //   is a multiple of 2^e G, a rounded product with any other constant k a multiple of ulp(k) G (ulp(k) =
    //   2^(ilogb k - 52)).  One time level therefore refines the grid by at most 2^er, and within a level the finest
    //   intermediate grid is 2^ew times the level's.  As long as every grid stays >= 2^-1074 no operation of either form
    //   loses a bit to the subnormal range:  eL - 52 + MAX_FUSE er + ew >= -1074  (one level of margin: MAX_FUSE - 1
    //   levels feed the last one).
    //   overflow: below fast_thr no level reaches 2^1022; lowering the screen by 2^(eh + 2), 2^eh the largest factor a
    //   difference is multiplied with in either form, keeps every product and F finite.
    p.slow_thr = p.p2_hi = p.p2_q = p.p2_k = 0.0;
    if (!contract && p.div_mode <= 1 && p.fast_thr > 0.0 && pow2(std::fabs(vx)) && pow2(std::fabs(vy)) && std::isfinite(p.kdiff) &&
        std::isfinite(p.mdt)) {
        const double A = p.div_mode == 1 ? vx * p.rdx : vx, B = p.div_mode == 1 ? vy * p.rdy : vy;
        if (pow2(std::fabs(A)) && pow2(std::fabs(B))) {
            const bool by_y = vy > 0.0 || vx < 0.0;  // the kernel's rule: SY == 1 || SX == 0
            const double q = by_y ? A / B : B / A, K = p.mdt * (by_y ? B : A);
            const int eA = std::ilogb(A), eB = std::ilogb(B), eq = std::ilogb(q);
            int e2 = 0, ew = std::min({0, eA, eB, eq, -eq}), eh = std::max({0, eA, eB, eq, -eq});
            if (p.div_mode == 1) {
                e2 = std::min({0, std::ilogb(p.rdx2), std::ilogb(p.rdy2)});
                ew = std::min({ew, e2, std::ilogb(p.rdx), std::ilogb(p.rdy)});
                eh = std::max({eh, std::ilogb(p.rdx), std::ilogb(p.rdy)});
            }
            int er = 0;
            if (p.kdiff != 0.0) er = std::min(er, std::ilogb(p.kdiff) - 52 + e2);
            if (p.mdt != 0.0) er = std::min(er, std::ilogb(p.mdt) - 52 + std::min(eA, eB));
            const int eL = -1074 + 52 - MAX_FUSE * er - ew;
            // generous bounds: a screen above 2^-300 would send ordinary far fields to the plain body; a q beyond
            // 2^+-100 is no velocity field anyone sweeps
            if (eL <= -300 && eh <= 100 && pow2(std::fabs(q)) && (K == 0.0 || std::isnormal(K))) {  // K: exact unless it underflows
                p.slow_thr = std::ldexp(1.0, eL);
                p.p2_hi = std::ldexp(p.fast_thr, -(eh + 2));
                p.p2_q = q;
                p.p2_k = K;
            }
        }
    }
    if (contract) p.div_mode = 3;
    return p;
}

// copies the partials the launch wrote and folds each member's in block order, starting from its first
int fold_partials(const double* scratch_dev, int rows, int kind, double* out, hipStream_t st, const Members& mb) {
    const size_t G = static_cast<size_t>(reduce_blocks(rows, mb.cap)), hi = G * mb.count;
    std::vector<double> h(kind == 0 ? 2 * hi : hi);
    CSIM_HIP(hipMemcpyAsync(h.data(), scratch_dev, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
    CSIM_HIP(hipStreamSynchronize(st));
    for (int m = 0; m < mb.count; ++m) {
        const double* p = h.data() + m * G;
        double r0 = p[0], r1 = kind == 0 ? p[hi] : 0.0;
        for (size_t k = 1; k < G; ++k) {
            if (kind == 0) {
                r0 = std::fmin(r0, p[k]);
                r1 = std::fmax(r1, p[hi + k]);
            } else if (kind == 1) {
                r0 += p[k];
            } else {
                r0 = max_nan(r0, p[k]);  // fmax would drop the NaN the kernel kept
            }
        }
        if (kind == 0) {
            out[2 * m] = r0;
            out[2 * m + 1] = r1;
        } else {
            out[m] = r0;
        }
    }
    return CSIM_OK;
}

int fold_checksum(const double* scratch_dev, int rows, unsigned long long* out, hipStream_t st, const Members& mb) {
    const size_t G = static_cast<size_t>(reduce_blocks(rows, mb.cap));
    std::vector<unsigned long long> h(G * mb.count);
    CSIM_HIP(hipMemcpyAsync(h.data(), scratch_dev, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, st));
    CSIM_HIP(hipStreamSynchronize(st));
    for (int m = 0; m < mb.count; ++m) {
        unsigned long long acc = 0;
        for (size_t k = 0; k < G; ++k) acc += h[m * G + k];
        out[m] = acc;
    }
    return CSIM_OK;
}

int upload_2d(double* d, int nx, int ny, int pitch, const double* host) {
    CSIM_HIP(hipMemcpy2D(d + (LPAD - 1), sizeof(double) * pitch, host, sizeof(double) * (nx + 2),
                         sizeof(double) * (nx + 2), ny + 2, hipMemcpyHostToDevice));
    return CSIM_OK;
}
int download_2d(const double* d, int nx, int ny, int pitch, double* host) {
    CSIM_HIP(hipMemcpy2D(host, sizeof(double) * (nx + 2), d + (LPAD - 1), sizeof(double) * pitch,
                         sizeof(double) * (nx + 2), ny + 2, hipMemcpyDeviceToHost));
    return CSIM_OK;
}
int download_interior_2d(const double* d, int nx, int ny, int pitch, double* host) {
    CSIM_HIP(hipMemcpy2D(host, sizeof(double) * nx, d + pitch + LPAD, sizeof(double) * pitch,
                         sizeof(double) * nx, ny, hipMemcpyDeviceToHost));
    return CSIM_OK;
}

// The 8 peers of a tile (L R B T BL BR TL TR): the four sides from the decomposition, a diagonal
// only where both adjacent sides have neighbours.  A size-1 decomposition whose sides were pointed
// at rank 0 is the self-linked test torus.
void neighbours8(const csim_decomp& dec, int nbr8[8]) {
    for (int k = 0; k < 4; ++k) nbr8[k] = dec.nbr[k];
    const int cx = dec.coords[0], cy = dec.coords[1], py = dec.dims[1];
    auto diag = [&](int sx, int sy, int dx_, int dy_) {
        if (dec.nbr[sx] < 0 || dec.nbr[sy] < 0) return -1;
        return dec.size == 1 ? 0 : (cx + dx_) * py + (cy + dy_);
    };
    nbr8[4] = diag(CSIM_LEFT, CSIM_BOTTOM, -1, -1);
    nbr8[5] = diag(CSIM_RIGHT, CSIM_BOTTOM, +1, -1);
    nbr8[6] = diag(CSIM_LEFT, CSIM_TOP, -1, +1);
    nbr8[7] = diag(CSIM_RIGHT, CSIM_TOP, +1, +1);
}

// doubles in the face of direction d at depth H on an nx x ny tile (depth 1: the interior span of an
// edge line, reference src/halo.cpp:12-18; deeper: ghost entries ride along, corners are H x H blocks)
size_t face_doubles(int d, int H, int nx, int ny) {
    if (H == 1) return d < 2 ? static_cast<size_t>(ny) : static_cast<size_t>(nx);
    return d < 2 ? static_cast<size_t>(H) * (ny + 2) : d < 4 ? static_cast<size_t>(H) * (nx + 2)
                                                       : static_cast<size_t>(H) * H;
}

bool valid_bc(const int bc[4]) {
    for (int s = 0; s < 4; ++s)
        if (bc[s] < CSIM_BC_DIRICHLET || bc[s] > CSIM_BC_PERIODIC) return false;
    return true;
}

}  // namespace csim

using namespace csim;

extern "C" {

const char* csim_last_error(void) { return g_err.c_str(); }

int csim_abi_version(void) { return CSIM_ABI_VERSION; }

int csim_device_count(int* count) {
    CSIM_REQUIRE(count, "count is null");
    CSIM_HIP(hipGetDeviceCount(count));
    return CSIM_OK;
}

int csim_set_device(int device) {
    CSIM_HIP(hipSetDevice(device));
    return CSIM_OK;
}

int csim_device_name(char* buf, size_t n) {
    CSIM_REQUIRE(buf && n > 0, "bad buffer");
    int dev = 0;
    CSIM_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    CSIM_HIP(hipGetDeviceProperties(&prop, dev));
    std::snprintf(buf, n, "%s", prop.gcnArchName);
    return CSIM_OK;
}

// reference include/stability.hpp:5-16
// host arithmetic only: what make_phys derives for option "pow2_v" (0 in out[0]: the form is off for these parameters)
int csim_pow2_velocity_screen(double dx, double dy, double D, double dt, double vx, double vy, double out[4]) {
    CSIM_REQUIRE(out, "null argument");
    const Phys p = make_phys(dx, dy, D, dt, vx, vy);
    out[0] = p.slow_thr, out[1] = p.p2_hi, out[2] = p.p2_q, out[3] = p.p2_k;
    return CSIM_OK;
}

// host arithmetic only: what a stepper with these parameters (and "pow2_v" on) asks of a field before it leases the
// screen for R steps — out[0] = M_req, out[1] = m_req (0: no lease of that kind), out[2] = eta, out[3] = a0
int csim_screen_lease_bounds(double dx, double dy, double D, double dt, double vx, double vy, long R, double out[4]) {
    CSIM_REQUIRE(out, "null argument");
    CSIM_REQUIRE(R >= 1, "R must be >= 1");
    const Phys p = make_phys(dx, dy, D, dt, vx, vy);
    const LeaseBounds b = lease_bounds(p, R);
    out[0] = b.M_req, out[1] = b.m_req, out[2] = b.eta, out[3] = p.a0;
    return CSIM_OK;
}

double csim_safe_dt(double dx, double dy, double vx, double vy, double D) {
    const double inf = std::numeric_limits<double>::infinity();
    const double ax = std::fabs(vx), ay = std::fabs(vy);
    const double rate = (ax > 0 ? ax / dx : 0.0) + (ay > 0 ? ay / dy : 0.0);
    const double dt_adv = rate > 0 ? 1.0 / rate : inf;
    const double w = 1.0 / (dx * dx) + 1.0 / (dy * dy);
    const double dt_diff = D > 0 ? 1.0 / (2.0 * D * w) : inf;
    return std::min(dt_adv, dt_diff);
}

// reference src/decomp.cpp:5-34 with MPI_Dims_create / MPI_Cart_* re-derived:
// most balanced factor pair, larger factor first; rank = coords[0]*dims[1] + coords[1].
int csim_decomp_init(int size, int rank, int nx_global, int ny_global, csim_decomp* out) {
    CSIM_REQUIRE(out, "out is null");
    CSIM_REQUIRE(size >= 1 && rank >= 0 && rank < size, "bad size/rank");
    CSIM_REQUIRE(nx_global > 0 && ny_global > 0, "nx/ny must be > 0");
    int small = 1;
    for (int f = 1; static_cast<long>(f) * f <= size; ++f)
        if (size % f == 0) small = f;
    csim_decomp d{};
    d.size = size;
    d.rank = rank;
    d.dims[0] = size / small;
    d.dims[1] = small;
    d.coords[0] = rank / d.dims[1];
    d.coords[1] = rank % d.dims[1];
    const int cx = d.coords[0], cy = d.coords[1];
    d.nbr[CSIM_LEFT] = cx > 0 ? (cx - 1) * d.dims[1] + cy : CSIM_NO_NEIGHBOR;
    d.nbr[CSIM_RIGHT] = cx + 1 < d.dims[0] ? (cx + 1) * d.dims[1] + cy : CSIM_NO_NEIGHBOR;
    d.nbr[CSIM_BOTTOM] = cy > 0 ? cx * d.dims[1] + (cy - 1) : CSIM_NO_NEIGHBOR;
    d.nbr[CSIM_TOP] = cy + 1 < d.dims[1] ? cx * d.dims[1] + (cy + 1) : CSIM_NO_NEIGHBOR;
    d.nx_global = nx_global;
    d.ny_global = ny_global;
    const int bx = nx_global / d.dims[0], by = ny_global / d.dims[1];
    d.nx_local = bx + (cx == d.dims[0] - 1 ? nx_global % d.dims[0] : 0);
    d.ny_local = by + (cy == d.dims[1] - 1 ? ny_global % d.dims[1] : 0);
    d.x_offset = cx * bx;
    d.y_offset = cy * by;
    CSIM_REQUIRE(d.nx_local > 0 && d.ny_local > 0, "more ranks than cells along an axis");
    *out = d;
    return CSIM_OK;
}

// THE message order of one halo exchange — the only place it is decided (post_exchange and
// post_exchange2 walk this plan).  Sends go out in direction order; receives are posted in
// opposite-direction order, so that the k-th message a rank sends to a given peer is the k-th one
// that peer expects from it even when one peer sits in several directions (2-wide process grids, the
// self-linked torus): RCCL matches the sends and receives of a pair in posting order.
int csim_exchange_plan(const csim_decomp* dec, int depth, csim_msg sends[8], int* nsend, csim_msg recvs[8],
                       int* nrecv) {
    CSIM_REQUIRE(dec && sends && nsend && recvs && nrecv, "null argument");
    CSIM_REQUIRE(depth >= 1 && depth <= MAX_FUSE, "depth must be 1..7");
    static const int recv_order1[4] = {CSIM_RIGHT, CSIM_LEFT, CSIM_TOP, CSIM_BOTTOM};
    static const int recv_order8[8] = {1, 0, 3, 2, 7, 6, 5, 4};
    int nbr8[8];
    neighbours8(*dec, nbr8);
    const int ndir = depth == 1 ? 4 : 8;
    const int* order = depth == 1 ? recv_order1 : recv_order8;
    int ns = 0, nr = 0;
    for (int d = 0; d < ndir; ++d)
        if (nbr8[d] >= 0)
            sends[ns++] = csim_msg{nbr8[d], d, static_cast<long>(face_doubles(d, depth, dec->nx_local, dec->ny_local))};
    for (int q = 0; q < ndir; ++q) {
        const int d = order[q];
        if (nbr8[d] >= 0)
            recvs[nr++] = csim_msg{nbr8[d], d, static_cast<long>(face_doubles(d, depth, dec->nx_local, dec->ny_local))};
    }
    *nsend = ns;
    *nrecv = nr;
    return CSIM_OK;
}

// ---- Field -------------------------------------------------------------------------------------
// what csim_field_create hands out: the handle of internal.hpp (its pointers are views) and the owners of its memory
struct FieldMem : csim_field {
    DeviceBuf mem, partials;
    void release() { mem.release(), partials.release(); }
};
static FieldMem* owner(csim_field* f) { return static_cast<FieldMem*>(f); }

static int field_alloc(FieldMem* f) {
    CSIM_TRY(f->mem.reserve(f->bytes()));
    CSIM_HIP(hipMemset(f->mem.p, 0, f->bytes()));
    CSIM_TRY(f->partials.reserve(sizeof(double) * 2 * REDUCE_BLOCKS));
    f->alloc = f->mem.as();
    f->d = f->alloc + static_cast<size_t>(GHOST_EXTRA) * f->pitch;
    f->scratch = f->partials.as();
    return CSIM_OK;
}

int csim_field_create(int nx, int ny, int halo, double dx, double dy, csim_field** out) {
    CSIM_REQUIRE(out, "out is null");
    *out = nullptr;
    CSIM_REQUIRE(nx > 0 && ny > 0, "nx/ny must be > 0");
    CSIM_REQUIRE(halo == 1, "only halo == 1 is supported (reference src/main.cpp:65)");
    CSIM_REQUIRE(dx > 0 && dy > 0, "dx/dy must be > 0");
    FieldMem* f = new FieldMem;
    f->nx = nx;
    f->ny = ny;
    f->halo = halo;
    f->dx = dx;
    f->dy = dy;
    f->pitch = pitch_for(nx);
    if (field_alloc(f) != CSIM_OK) {
        const std::string why = g_err;
        csim_field_destroy(f);
        return fail(CSIM_ERR_HIP, "csim_field_create: " + why);
    }
    *out = f;
    return CSIM_OK;
}

int csim_field_destroy(csim_field* f) {
    if (!f) return CSIM_OK;
    owner(f)->release();
    delete owner(f);
    return CSIM_OK;
}

int csim_field_upload(csim_field* f, const double* host) {
    CSIM_REQUIRE(f && host, "null argument");
    return upload_2d(f->d, f->nx, f->ny, f->pitch, host);
}

int csim_field_download(const csim_field* f, double* host) {
    CSIM_REQUIRE(f && host, "null argument");
    return download_2d(f->d, f->nx, f->ny, f->pitch, host);
}

int csim_field_download_interior(const csim_field* f, double* host) {
    CSIM_REQUIRE(f && host, "null argument");
    return download_interior_2d(f->d, f->nx, f->ny, f->pitch, host);
}

int csim_field_fill(csim_field* f, double value) {
    CSIM_REQUIRE(f, "null field");
    CSIM_HIP(launch_fill(f->d, f->nx, f->ny, f->pitch, value, nullptr));
    CSIM_HIP(hipStreamSynchronize(nullptr));
    return CSIM_OK;
}

static bool same_shape(const csim_field* a, const csim_field* b) {
    return a && b && a->nx == b->nx && a->ny == b->ny;
}

int csim_field_copy(csim_field* dst, const csim_field* src) {
    CSIM_REQUIRE(same_shape(dst, src), "fields differ in shape");
    CSIM_HIP(hipMemcpy(dst->alloc, src->alloc, src->bytes(), hipMemcpyDeviceToDevice));
    return CSIM_OK;
}

int csim_field_swap(csim_field* a, csim_field* b) {
    CSIM_REQUIRE(same_shape(a, b), "fields differ in shape");
    std::swap(owner(a)->mem, owner(b)->mem);
    std::swap(a->alloc, b->alloc);
    std::swap(a->d, b->d);
    return CSIM_OK;
}

int csim_field_minmax(const csim_field* f, double out[2]) {
    CSIM_REQUIRE(f && out, "null argument");
    CSIM_HIP(launch_minmax(f->d, f->nx, f->ny, f->pitch, f->scratch, nullptr));
    return fold_partials(f->scratch, f->ny + 2, 0, out, nullptr);
}

int csim_field_sum(const csim_field* f, double* out) {
    CSIM_REQUIRE(f && out, "null argument");
    CSIM_HIP(launch_sum(f->d, f->nx, f->ny, f->pitch, f->scratch, nullptr));
    return fold_partials(f->scratch, f->ny, 1, out, nullptr);
}

int csim_field_linf_diff(const csim_field* a, const csim_field* b, double* out) {
    CSIM_REQUIRE(same_shape(a, b) && out, "fields differ in shape");
    CSIM_HIP(launch_linf(a->d, b->d, a->nx, a->ny, a->pitch, a->scratch, nullptr));
    return fold_partials(a->scratch, a->ny, 2, out, nullptr);
}

// ---- operators ----------------------------------------------------------------------------------
int csim_apply_boundary(csim_field* f, const int bc[4], const int is_physical[4], double value) {
    CSIM_REQUIRE(f && bc && is_physical, "null argument");
    CSIM_REQUIRE(valid_bc(bc), "unknown boundary type");
    GhostArgs g{};
    for (int s = 0; s < 4; ++s) {
        g.bc[s] = bc[s];
        g.phys[s] = is_physical[s] != 0;
        g.recv[s] = nullptr;
    }
    g.value = value;
    CSIM_HIP(launch_ghost_fill(f->d, nullptr, f->nx, f->ny, f->pitch, g, nullptr));
    CSIM_HIP(hipStreamSynchronize(nullptr));
    return CSIM_OK;
}

int csim_diffusion_step(const csim_field* u, csim_field* out, double D, double dt) {
    CSIM_REQUIRE(same_shape(u, out), "fields differ in shape");
    CSIM_REQUIRE(u->d != out->d, "u and out must be distinct fields");
    const Phys p = make_phys(u->dx, u->dy, D, dt, 0.0, 0.0);
    CSIM_HIP(launch_diffusion_only(u->d, out->d, u->nx, u->ny, u->pitch, p, nullptr));
    CSIM_HIP(launch_ring_copy(u->d, out->d, u->nx, u->ny, u->pitch, nullptr));
    CSIM_HIP(hipStreamSynchronize(nullptr));
    return CSIM_OK;
}

int csim_advection_step(const csim_field* u, csim_field* out, double vx, double vy, double dt) {
    CSIM_REQUIRE(same_shape(u, out), "fields differ in shape");
    CSIM_REQUIRE(u->d != out->d, "u and out must be distinct fields");
    const Phys p = make_phys(u->dx, u->dy, 0.0, dt, vx, vy);
    CSIM_HIP(launch_advection_only(u->d, out->d, u->nx, u->ny, u->pitch, p, nullptr));
    CSIM_HIP(hipStreamSynchronize(nullptr));
    return CSIM_OK;
}

int csim_fused_step(const csim_field* u, csim_field* out, double D, double dt, double vx, double vy) {
    CSIM_REQUIRE(same_shape(u, out), "fields differ in shape");
    CSIM_REQUIRE(u->d != out->d, "u and out must be distinct fields");
    const Phys p = make_phys(u->dx, u->dy, D, dt, vx, vy);
    SweepCfg cfg;
    CSIM_HIP(launch_ring_copy(u->d, out->d, u->nx, u->ny, u->pitch, nullptr));
    CSIM_HIP(launch_sweep(u->d, out->d, u->nx, u->ny, u->pitch, p, cfg, nullptr));
    CSIM_HIP(hipStreamSynchronize(nullptr));
    return CSIM_OK;
}

}  // extern "C"
