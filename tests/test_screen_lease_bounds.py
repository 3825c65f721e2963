"""The screen lease's bounds (stepper option "screen_lease", csim_screen_lease_bounds = lease_bounds in csrc/api.cpp) on
the CPU, without a GPU.

The bound: a numpy float64 model of the cell update in the reference's operation order (numpy evaluates every
elementwise operation in IEEE double, one rounding each, nothing contracted) steps random strictly positive fields whose
exponents differ by hundreds of binades from cell to cell, inside rings of +0 and of positive values, and at every step
min|u| and max|u| must stay within what the bounds promise: max <= max0 g^n, min >= min0 (a0 (1 - eta))^n, hence inside
[2 L, upper) for R + 7 steps when the field starts inside [m_req, M_req].

Identity under the lease: for such fields — admitted by a restatement of the verdict, here, on the model alone — the
12-operation form (a small C restatement, it needs fma) equals the reference form bit for bit over R + 7 steps."""
import ctypes as C
import math
import shutil
import subprocess

import numpy as np
import pytest

from __graft_entry__ import load_package

MAX_FUSE = 7
NX, NY = 40, 28

# (D, dt, vx, vy, dx, dy), every stencil coefficient positive: the bench's; a power-of-two spacing (DIV 1); the other
# upwind sign pairs; close to the stability limit (a0 = 0.05); another velocity pair
POSITIVE = [(0.05, 0.1, 0.5, 0.25, 1.0, 1.0), (0.05, 0.01, 0.5, 0.25, 0.5, 0.25), (0.05, 0.1, -0.5, 0.25, 1.0, 1.0),
            (0.05, 0.1, 0.5, -0.25, 1.0, 1.0), (0.05, 0.1, -0.5, -0.25, 1.0, 1.0), (0.05, 1.0, 0.5, 0.25, 1.0, 1.0),
            (0.05, 0.1, 1.0, 0.125, 1.0, 1.0)]
# a coefficient that is zero (no diffusion: nothing multiplies the downwind neighbour) or negative (beyond the limit)
NOT_POSITIVE = [(0.0, 0.1, 0.5, 0.25, 1.0, 1.0), (0.05, 2.0, 0.5, 0.25, 1.0, 1.0), (0.05, 1.2, 0.5, 0.25, 1.0, 1.0)]
IDS = lambda t: "D%g_dt%g_v%g_%g_d%g_%g" % t  # noqa: E731


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


def step_ref(u, D, dt, vx, vy, dx, dy):
    """one step of the interior in the reference's operation order (src/diffusion.cpp:9-16, src/advection.cpp:13-33);
    the ring keeps its values"""
    c, W, E, S, N = u[1:-1, 1:-1], u[1:-1, :-2], u[1:-1, 2:], u[:-2, 1:-1], u[2:, 1:-1]
    tc = 2.0 * c
    lap = ((E - tc) + W) / (dx * dx) + ((N - tc) + S) / (dy * dy)
    o = c + (dt * D) * lap
    dudx = (c - W) / dx if vx >= 0 else (E - c) / dx
    dudy = (c - S) / dy if vy >= 0 else (N - c) / dy
    adv = vx * dudx + vy * dudy
    out = u.copy()
    out[1:-1, 1:-1] = o + (-dt) * adv
    return out


def growth(D, dt, vx, vy, dx, dy):
    return (1.0 + 4.0 * dt * D * (1 / dx ** 2 + 1 / dy ** 2) + 2.0 * dt * (abs(vx) / dx + abs(vy) / dy)) * (1.0 + 1e-9)


def fields(rng, lo, hi, ring):
    """positive fields with exponents in [lo, hi]: independent per cell; a smooth ramp with cell-to-cell noise; the
    smallest value in the inflow corners, where nothing feeds it"""
    span = hi - lo
    for kind in range(3):
        e = rng.integers(lo, hi + 1, size=(NY + 2, NX + 2))
        if kind == 1:
            e = lo + (np.add.outer(np.arange(NY + 2), np.arange(NX + 2)) * span) // (NX + NY + 2)
            e = np.clip(e + rng.integers(-3, 4, size=e.shape), lo, hi)
        if kind == 2:
            e[:4, :4] = e[:4, -4:] = e[-4:, :4] = e[-4:, -4:] = lo
        m = rng.integers(2 ** 52, 2 ** 53, size=e.shape).astype(np.float64)
        u = np.ldexp(m, (e - 52).astype(np.int32))
        u[u > 2.0 ** hi] = 2.0 ** hi   # (mantissas run up to 2 - ulp)
        if ring == "zero":
            u[0, :] = u[-1, :] = u[:, 0] = u[:, -1] = 0.0
        yield np.ascontiguousarray(u)


def admits(u, M_req, m_req):
    """the verdict's rule for a positive field, restated: bit 0 and bit 1 (kernels.hip, lease_verdict)"""
    inner, a = u[1:-1, 1:-1], np.abs(u)
    nz = a[a != 0]
    ring = np.concatenate([u[0], u[-1], u[1:-1, 0], u[1:-1, -1]])
    upper = M_req > 0 and np.isfinite(u).all() and nz.max() <= M_req
    one_sign = (inner > 0).all() and not (ring < 0).any() and not (np.signbit(ring) & (ring == 0)).any()
    return bool(upper), bool(upper and m_req > 0 and one_sign and nz.min() >= m_req)


@pytest.mark.parametrize("phys", POSITIVE, ids=IDS)
@pytest.mark.parametrize("ring", ["zero", "positive"])
def test_min_and_max_stay_within_the_promise(csim, phys, ring):
    D, dt, vx, vy, dx, dy = phys
    R = 48
    M_req, m_req, eta, a0 = csim.screen_lease_bounds(D, dt, vx, vy, dx, dy, R)
    L, upper = csim.pow2_velocity_screen(D, dt, vx, vy, dx, dy)[:2]
    assert L > 0 and M_req > 0 and m_req > 0, "these parameters lease the 12-operation body"
    assert 0 < eta <= 2.0 ** -20 and 0 < a0 < 1
    assert math.frexp(M_req)[0] == 0.5 and math.frexp(m_req)[0] == 0.5       # powers of two
    g, shrink = growth(*phys), a0 * (1.0 - eta)
    n_all = R + MAX_FUSE
    # what the bounds promise in one line each (in logarithms: g^n itself may overflow)
    assert math.log2(M_req) + n_all * math.log2(g) < math.log2(upper)
    assert math.log2(m_req) + n_all * math.log2(shrink) > math.log2(2.0 * L)
    e_lo, e_hi = int(math.log2(m_req)), int(math.log2(M_req))
    assert e_hi - e_lo > 700
    rng = np.random.default_rng(11)
    for lo, hi in [(e_lo, e_lo + 600), (e_hi - 600, e_hi), (e_lo, e_hi)]:
        for u in fields(rng, lo, hi, ring):
            assert admits(u, M_req, m_req) == (True, True)
            a = np.abs(u)
            max0, min0 = a.max(), a[a != 0].min()
            with np.errstate(over="raise", invalid="raise"):
                for n in range(1, n_all + 1):
                    u = step_ref(u, D, dt, vx, vy, dx, dy)
                    inner = u[1:-1, 1:-1]
                    assert (inner > 0).all(), (n, "an interior zero or a sign change")
                    assert math.log2(inner.max()) <= math.log2(max0) + n * math.log2(g), n
                    assert math.log2(inner.min()) >= math.log2(min0) + n * math.log2(shrink), n
                    assert 2.0 * L <= inner.min() and inner.max() < upper, n


@pytest.mark.parametrize("phys", NOT_POSITIVE, ids=IDS)
def test_no_p2_lease_without_positive_coefficients(csim, phys):
    D, dt, vx, vy, dx, dy = phys
    assert csim.pow2_velocity_screen(D, dt, vx, vy, dx, dy)[0] > 0, "the 12-operation form itself is on"
    M_req, m_req, eta, _ = csim.screen_lease_bounds(D, dt, vx, vy, dx, dy, 16)
    assert M_req > 0 and m_req == 0.0 and eta == 0.0


def test_general_velocities_lease_the_upper_bound_only(csim):
    M_req, m_req = csim.screen_lease_bounds(0.05, 0.1, 0.3, 0.2, 1.0, 1.0, 1024)[:2]
    assert M_req > 2.0 ** 200 and m_req == 0.0
    # IEEE division and parameters far from stable: no screened body, no lease
    assert csim.screen_lease_bounds(0.05, 0.1, 0.5, 0.25, 0.3, 0.7, 1024)[:2] == (0.0, 0.0)
    assert csim.screen_lease_bounds(3.0e18, 1.0, 0.5, 0.25, 1.0, 1.0, 1024)[:2] == (0.0, 0.0)


def test_the_bench_field_is_admitted_for_the_default_lease(csim):
    """bench.py's hotspot exp(-r^2 / (2 sigma^2)), sigma = 0.05 of the domain: 1 at the centre, exp(-100) in the corners"""
    M_req, m_req = csim.screen_lease_bounds(0.05, 0.1, 0.5, 0.25, 1.0, 1.0, 1024)[:2]
    assert m_req < math.exp(-100.0) and 1.0 < M_req
    assert 2.0 ** -470 < m_req < 2.0 ** -430


# ---- identity under the lease ---------------------------------------------------------------------------------------
SRC = r"""
#include <math.h>
#include <string.h>
typedef struct { double kdiff, mdt, vx, vy, rdx, rdy, rdx2, rdy2, q, K; int div, sx, sy; } P;
static double ref_cell(double c, double W, double E, double S, double N, const P* p) {
    const double tc = 2.0 * c;
    double lx = (E - tc) + W, ly = (N - tc) + S;
    if (p->div) { lx = lx * p->rdx2; ly = ly * p->rdy2; }
    const double lap = lx + ly;
    const double o = c + p->kdiff * lap;
    double gx = p->sx ? c - W : E - c, gy = p->sy ? c - S : N - c;
    if (p->div) { gx = gx * p->rdx; gy = gy * p->rdy; }
    const double adv = p->vx * gx + p->vy * gy;
    return o + p->mdt * adv;
}
static double p2_cell(double c, double W, double E, double S, double N, const P* p) {
    double lx = fma(-2.0, c, E) + W, ly = fma(-2.0, c, N) + S;
    if (p->div) { lx = lx * p->rdx2; ly = ly * p->rdy2; }
    const double lap = lx + ly;
    const double o = c + p->kdiff * lap;
    const double gx = p->sx ? c - W : E - c, gy = p->sy ? c - S : N - c;
    const double F = (p->sy || !p->sx) ? fma(p->q, gx, gy) : fma(p->q, gy, gx);
    return o + p->K * F;
}
/* `steps` steps of an (ny + 2) x (nx + 2) field with a held ring, both ways, each form on its own state; returns the
   number of interior cells whose bits differ, summed over the steps; mins[n] = the reference form's interior minimum */
long march(int nx, int ny, int steps, const double* u0, const P* p, double* a, double* b, double* mins) {
    const int w = nx + 2;
    const size_t n = (size_t)w * (ny + 2);
    long bad = 0;
    double* ra = a; double* rb = a + n; double* pa = b; double* pb = b + n;
    memcpy(ra, u0, sizeof(double) * n); memcpy(rb, u0, sizeof(double) * n);
    memcpy(pa, u0, sizeof(double) * n); memcpy(pb, u0, sizeof(double) * n);
    for (int s = 0; s < steps; ++s) {
        double mn = INFINITY;
        for (int j = 1; j <= ny; ++j)
            for (int i = 1; i <= nx; ++i) {
                const int k = j * w + i;
                rb[k] = ref_cell(ra[k], ra[k - 1], ra[k + 1], ra[k - w], ra[k + w], p);
                pb[k] = p2_cell(pa[k], pa[k - 1], pa[k + 1], pa[k - w], pa[k + w], p);
                if (memcmp(&rb[k], &pb[k], sizeof(double)) != 0) ++bad;
                if (rb[k] < mn) mn = rb[k];
            }
        mins[s] = mn;
        double* t = ra; ra = rb; rb = t;
        t = pa; pa = pb; pb = t;
    }
    return bad;
}
"""


class P(C.Structure):
    _fields_ = [(k, C.c_double) for k in "kdiff mdt vx vy rdx rdy rdx2 rdy2 q K".split()] + \
               [(k, C.c_int) for k in "div sx sy".split()]


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "a C compiler is needed"
    d = tmp_path_factory.mktemp("lease")
    (d / "forms.c").write_text(SRC)
    so = d / "libforms.so"
    subprocess.run([cc, "-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", str(so),
                    str(d / "forms.c"), "-lm"], check=True)
    lib = C.CDLL(str(so))
    dp = C.POINTER(C.c_double)
    lib.march.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.POINTER(P), dp, dp, dp]
    lib.march.restype = C.c_long
    return lib


@pytest.mark.parametrize("phys", POSITIVE, ids=IDS)
@pytest.mark.parametrize("ring", ["zero", "positive"])
def test_forms_agree_under_the_lease(csim, forms, phys, ring):
    D, dt, vx, vy, dx, dy = phys
    R = 16
    M_req, m_req = csim.screen_lease_bounds(D, dt, vx, vy, dx, dy, R)[:2]
    L, _, q, K = csim.pow2_velocity_screen(D, dt, vx, vy, dx, dy)
    assert m_req > 0
    p = P(kdiff=dt * D, mdt=-dt, vx=vx, vy=vy, rdx=1 / dx, rdy=1 / dy, rdx2=1 / (dx * dx), rdy2=1 / (dy * dy), q=q, K=K,
          div=int((dx, dy) != (1.0, 1.0)), sx=int(vx >= 0), sy=int(vy >= 0))
    e_lo, e_hi = int(math.log2(m_req)), int(math.log2(M_req))
    rng = np.random.default_rng(5)
    steps = R + MAX_FUSE
    dp = C.POINTER(C.c_double)
    for lo, hi in [(e_lo, e_lo), (e_lo, e_lo + 300), (e_hi - 300, e_hi), (e_lo, e_hi)]:
        for u in fields(rng, lo, hi, ring):
            assert admits(u, M_req, m_req) == (True, True)      # the model alone admits it
            a, b, mins = np.empty(2 * u.size), np.empty(2 * u.size), np.empty(steps)
            bad = forms.march(NX, NY, steps, u.ctypes.data_as(dp), C.byref(p), a.ctypes.data_as(dp), b.ctypes.data_as(dp),
                              mins.ctypes.data_as(dp))
            assert bad == 0, (lo, hi)
            assert (mins >= 2.0 * L).all()


def test_forms_differ_below_the_lower_bound(csim, forms):
    """not vacuous: the same march from fields deep in the subnormal range — which the verdict refuses — shows mismatches"""
    D, dt, vx, vy, dx, dy = POSITIVE[0]
    M_req, m_req = csim.screen_lease_bounds(D, dt, vx, vy, dx, dy, 16)[:2]
    L, _, q, K = csim.pow2_velocity_screen(D, dt, vx, vy, dx, dy)
    p = P(kdiff=dt * D, mdt=-dt, vx=vx, vy=vy, rdx=1.0, rdy=1.0, rdx2=1.0, rdy2=1.0, q=q, K=K, div=0, sx=1, sy=1)
    dp = C.POINTER(C.c_double)
    u = next(fields(np.random.default_rng(3), -1074 + 52, -1020, "zero"))
    assert admits(u, M_req, m_req) == (True, False)
    a, b, mins = np.empty(2 * u.size), np.empty(2 * u.size), np.empty(4)
    assert forms.march(NX, NY, 4, u.ctypes.data_as(dp), C.byref(p), a.ctypes.data_as(dp), b.ctypes.data_as(dp),
                       mins.ctypes.data_as(dp)) > 0
