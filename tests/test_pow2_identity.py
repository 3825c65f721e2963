"""The 12-operation cell update for power-of-two velocities (stepper option "pow2_v") against the reference's 14
operations, on the CPU: a small C restatement of both forms (csrc/sweep_core.hpp: cell<.., FAST, P2> and the plain
sequence), compiled without FMA contraction like the oracle, marched over MAX_FUSE time levels of small tiles.

The screen's lower bound L and the constants q, K come from the library's own host arithmetic
(csim_pow2_velocity_screen = make_phys), so the test checks the derivation that ships: tiles whose values are all
exactly zero or at least L in magnitude must agree bit for bit at every level, for all four sign pairs (with the rule
which velocity is factored out), with and without power-of-two grid spacings — and tiles deep in the subnormal range
must NOT agree, so that the test cannot pass vacuously."""
import ctypes as C
import math
import shutil
import subprocess

import numpy as np
import pytest

from __graft_entry__ import load_package

LEVELS = 7  # MAX_FUSE
N = 96      # tile edge; level l is compared on [l, N - l)

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
/* levels 1..L of an n x n tile both ways (the border keeps its value); out: L tiles each */
void march(int n, int L, const double* u0, const P* p, double* ref, double* p2) {
    for (int form = 0; form < 2; ++form) {
        double* out = form ? p2 : ref;
        const double* in = u0;
        for (int l = 0; l < L; ++l) {
            double* o = out + (size_t)l * n * n;
            memcpy(o, in, sizeof(double) * n * n);
            for (int j = 1; j < n - 1; ++j)
                for (int i = 1; i < n - 1; ++i) {
                    const double c = in[j * n + i], W = in[j * n + i - 1], E = in[j * n + i + 1];
                    const double S = in[(j - 1) * n + i], Nn = in[(j + 1) * n + i];
                    o[j * n + i] = form ? p2_cell(c, W, E, S, Nn, p) : ref_cell(c, W, E, S, Nn, p);
                }
            in = o;
        }
    }
}
"""


class P(C.Structure):
    _fields_ = [(k, C.c_double) for k in "kdiff mdt vx vy rdx rdy rdx2 rdy2 q K".split()] + \
               [(k, C.c_int) for k in "div sx sy".split()]


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "a C compiler is needed"
    d = tmp_path_factory.mktemp("pow2")
    (d / "forms.c").write_text(SRC)
    so = d / "libforms.so"
    subprocess.run([cc, "-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", str(so),
                    str(d / "forms.c"), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.march.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(P), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.march.restype = None
    return lib


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


# (D, dt, |vx|, |vy|, dx, dy): the bench / shipped configurations, the other velocity pairs of the GPU test, power-of-two
# spacings finer and coarser than 1 (DIV 1), no diffusion, a tiny time step
PHYSICS = [(0.05, 0.1, 0.5, 0.25, 1.0, 1.0), (0.05, 0.1, 1.0, 0.125, 1.0, 1.0), (0.05, 0.05, 2.0, 0.5, 1.0, 1.0),
           (0.05, 0.01, 0.5, 0.25, 0.5, 0.25), (0.05, 0.1, 0.5, 0.25, 2.0, 4.0), (0.0, 0.1, 0.25, 0.5, 1.0, 1.0),
           (0.3, 1e-9, 0.5, 0.25, 1.0, 1.0)]
SIGNS = [(1, 1), (1, -1), (-1, 1), (-1, -1)]


def phys_struct(csim, D, dt, vx, vy, dx, dy):
    L, hi, q, K = csim.pow2_velocity_screen(D, dt, vx, vy, dx, dy)
    assert L > 0.0 and hi > 2.0 ** 700, (D, dt, vx, vy, dx, dy)
    assert math.frexp(L)[0] == 0.5 and L <= 2.0 ** -300          # a power of two, far below any ordinary field
    div = int((dx, dy) != (1.0, 1.0))
    p = P(kdiff=dt * D, mdt=-dt, vx=vx, vy=vy, rdx=1 / dx, rdy=1 / dy, rdx2=1 / (dx * dx), rdy2=1 / (dy * dy), q=q, K=K,
          div=div, sx=int(vx >= 0), sy=int(vy >= 0))
    # the factoring rule of cell<.., P2>: a positive velocity where there is one, vy first
    A, B = vx / dx, vy / dy
    by_y = vy > 0 or vx < 0
    assert q == (A / B if by_y else B / A) and K == -dt * (B if by_y else A)
    assert (B if by_y else A) > 0 or (vx < 0 and vy < 0)
    return p, L


def tile(rng, e_lo, e_hi, zeros, neg_zero):
    """n x n doubles of magnitude 2^e, e in [e_lo, e_hi] per 16 x 16 block: in half of the blocks neighbours differ by a few
    units of the last place only (the differences cancel down to the grid the values lie on), in the others mantissas
    are independent; blocks of equal values, exact zeros and (neg_zero) -0.0 are mixed in"""
    nb = N // 16
    e = rng.integers(e_lo, e_hi + 1, size=(nb, nb)).repeat(16, 0).repeat(16, 1)
    base = rng.integers(2 ** 52, 2 ** 53 - 64, size=(nb, nb)).repeat(16, 0).repeat(16, 1)
    near = rng.integers(0, 2, size=(nb, nb)).repeat(16, 0).repeat(16, 1).astype(bool)
    m = np.where(near, base + rng.integers(-8, 9, size=(N, N)), rng.integers(2 ** 52, 2 ** 53, size=(N, N)))
    flat = rng.integers(0, 8, size=(nb, nb)).repeat(16, 0).repeat(16, 1) == 0   # blocks of one value: every difference is 0
    m = np.where(flat, base, m)
    sign = np.where(rng.integers(0, 4, size=(nb, nb)).repeat(16, 0).repeat(16, 1) == 0, rng.choice([-1.0, 1.0], size=(N, N)), 1.0)
    u = np.ldexp(m.astype(np.float64), (e - 52).astype(np.int32)) * sign
    if zeros:
        z = rng.integers(0, 12, size=(N, N))
        u[z == 0] = 0.0
        u[40:52, 8:30] = 0.0
        if neg_zero:
            u[z == 1] = -0.0
            u[60:70, 50:60] = -0.0
    return np.ascontiguousarray(u)


def mismatches(forms, u, p):
    ref = np.empty((LEVELS, N, N))
    p2 = np.empty((LEVELS, N, N))
    forms.march(N, LEVELS, u.ctypes.data_as(C.POINTER(C.c_double)), C.byref(p), ref.ctypes.data_as(C.POINTER(C.c_double)),
                p2.ctypes.data_as(C.POINTER(C.c_double)))
    bad = 0
    for l in range(LEVELS):  # the border is held, so level l + 1 is a pure stencil result on [l + 1, N - l - 1)
        a, b = ref[l, l + 1:N - l - 1, l + 1:N - l - 1], p2[l, l + 1:N - l - 1, l + 1:N - l - 1]
        assert not np.isnan(a).any()
        bad += int((a.view(np.int64) != b.view(np.int64)).sum())
    return bad


@pytest.mark.parametrize("phys", PHYSICS, ids=lambda t: "D%g_dt%g_v%g_%g_d%g_%g" % t)
@pytest.mark.parametrize("sx,sy", SIGNS)
def test_forms_agree_at_and_above_L(forms, csim, phys, sx, sy):
    D, dt, vx, vy, dx, dy = phys
    p, L = phys_struct(csim, D, dt, sx * vx, sy * vy, dx, dy)
    eL = math.frexp(L)[1] - 1
    assert 2.0 ** eL == L
    both_negative = sx < 0 and sy < 0   # that flavour's screen also rejects a loaded -0 (see cell)
    bands = [(eL, eL), (eL, eL + 40), (-560, -520), (-40, 10), (600, 640)]
    if eL + 40 < -600:
        bands.append((-1010, -990))   # normal, but products with the small constants are subnormal: covered by L or not at all
    for k, (lo, hi) in enumerate(bands):
        if lo < eL:
            continue
        for seed in range(3):
            rng = np.random.default_rng(1000 * k + seed)
            u = tile(rng, lo, hi, zeros=seed > 0, neg_zero=not both_negative)
            assert (np.abs(u[u != 0]) >= L).all()
            assert mismatches(forms, u, p) == 0, (lo, hi, seed)


def test_forms_differ_in_the_subnormal_range(forms, csim):
    """without the lower screen the identity is false: the deep band must show mismatches (and L must lie above it)"""
    total = 0
    for sx, sy in SIGNS:
        p, L = phys_struct(csim, 0.05, 0.1, sx * 0.5, sy * 0.25, 1.0, 1.0)
        assert L > 2.0 ** -1000
        for seed in range(2):
            u = tile(np.random.default_rng(77 + seed), -1074 + 52, -1000, zeros=False, neg_zero=False)
            n = mismatches(forms, u, p)
            assert n > 0, (sx, sy, seed)
            total += n
    assert total > 100


def test_the_bench_field_passes_the_screen(csim):
    """bench.py's hotspot is A exp(-r^2 / (2 sigma^2)) with sigma = 0.05 of the domain and the centre in the middle: the
    far corner is exp(-(0.5^2 + 0.5^2) / (2 * 0.05^2)) = exp(-100), about 2^-144, and no interior cell is zero"""
    L = csim.pow2_velocity_screen(0.05, 0.1, 0.5, 0.25)[0]
    assert 2.0 ** -620 <= L <= 2.0 ** -580
    assert math.exp(-100.0) > 2.0 ** -145 > L


@pytest.mark.parametrize("sx,sy", SIGNS)
def test_zero_signs_and_exact_cancellation(forms, csim, sx, sy):
    """vx gx = -vy gy exactly (the sum cancels to a zero whose sign the factoring must keep), zero differences of both
    signs, and cells that are themselves +0 / -0: o + m must come out the same, sign of zero included"""
    vx, vy = sx * 0.5, sy * 0.25
    p, L = phys_struct(csim, 0.0, 0.1, vx, vy, 1.0, 1.0)   # D = 0: o = c + 0 * lap keeps a -0 alive as far as it can
    both_negative = sx < 0 and sy < 0
    u = np.zeros((N, N))
    j, i = np.mgrid[0:N, 0:N]
    # a plane a i + b j has gx = a, gy = b everywhere (either upwind side): vx a + vy b = 0 for b = -(vx / vy) a
    for k, a in enumerate([1.0, -3.0, 2.0 ** -200, 1.0 + 2.0 ** -52]):
        rows = slice(12 * k, 12 * k + 12)
        u[rows] = (a * i + (-(vx / vy) * a) * j)[rows]
    u[48:60] = 5.0          # constant: every difference +0
    u[60:72] = 0.0
    if not both_negative:
        u[72:84] = -0.0     # -0 everywhere: o = -0, m = +-0
        u[84:96, ::2] = -0.0
    assert mismatches(forms, u, p) == 0
    pd, _ = phys_struct(csim, 0.05, 0.1, vx, vy, 1.0, 1.0)
    assert mismatches(forms, u, pd) == 0
