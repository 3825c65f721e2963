"""numpy restatements of csim_ensemble_dot and csim_ensemble_obs_impact_global, written from the text of include/csim.h:
the dot in the class order of the Gram sum, an exact reference of it with its derived bound, and the global impact with
its summary.  On top of tests/espace_restatement.py (perturbations, the plan) and tests/impact_restatement.py (the
capture, the summary) by import only.  tests/test_impact_global_host.py pins them without a device;
tests/test_gpu_impact_global.py uses them as the reference of the kernels.

Every restatement does one rounded numpy operation per operation of the definition (numpy never contracts a * b + c),
so the GPU result can be compared bit for bit."""
import math
from fractions import Fraction

import numpy as np

import espace_restatement as espace
import impact_restatement as impact

SEG = espace.SEG
U = espace.U
MAX_FIELDS = 16
USED = impact.USED


def as_fields(fields):
    f = np.asarray(fields, dtype=np.float64)
    return f[None] if f.ndim == 2 else f


def dot(X, fields, t=None, centered=True):
    """(M, K) of csim_ensemble_dot on the members X (B, ny+2, nx+2): class partials as running sums over the class's
    cells in increasing e, folded in class order starting from partial 0.  Vectorised over the classes and the M x K
    block, a loop over trips x 64 cells, as espace_restatement.gram"""
    p, _ = espace.perturbations(X, t, centered)
    P = espace.interior_rows(p)
    F = espace.interior_rows(as_fields(fields))
    M, cells = P.shape
    K = F.shape[0]
    ny, nx = X.shape[1] - 2, X.shape[2] - 2
    nseg, Gc = espace.gram_plan(M, nx, ny)
    acc = np.zeros((Gc, M, K))
    term = np.empty((Gc, M, K))
    with np.errstate(all="ignore"):
        for trip in range(-(-nseg // Gc)):
            for c in range(SEG):
                first = trip * Gc * SEG + c
                if first >= cells:
                    break
                n = min(Gc, (cells - 1 - first) // SEG + 1)
                v = P[:, first:first + n * SEG:SEG].T  # (n, M): class g's cell c of this trip
                w = F[:, first:first + n * SEG:SEG].T  # (n, K)
                np.multiply(v[:, :, None], w[:, None, :], out=term[:n])
                np.add(acc[:n], term[:n], out=acc[:n])
        out = acc[0]
        for g in range(1, Gc):
            out = out + acc[g]
    return out


def dot_exact(P, F):
    """the exact sums of the rows of P (M, cells) against the rows of F (K, cells), as Fractions"""
    fp = [[Fraction(float(v)) for v in row] for row in P]
    ff = [[Fraction(float(v)) for v in row] for row in F]
    return [[sum((a * b for a, b in zip(pk, fr)), Fraction(0)) for fr in ff] for pk in fp]


def dot_bound(P, F, nx, ny, M=None):
    """gamma_k sum |p_k f_r| per entry with the k of espace_restatement.gram_bound: one rounding of the product, at most
    (cells of its class) additions of the class's running sum and Gc - 1 of the fold.  Derived, not tuned.  M: the
    forecast members of the sum, which decide the classes, when P holds only some of their rows"""
    M = P.shape[0] if M is None else M
    _, Gc = espace.gram_plan(M, nx, ny)
    ku = (1 + espace.class_cells(M, nx, ny) + (Gc - 1)) * U
    A, B = np.abs(P), np.abs(F)
    return ku / (1.0 - ku) * np.array([[math.fsum((a * b).tolist()) for b in B] for a in A])


def value(a, g, dn):
    """J of one observation: c = +0; c = c + a_k * g_k (k in order); S = c / (M-1); J = dn * S"""
    a, g = np.asarray(a, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(all="ignore"):
        c = np.float64(0.0)
        for ak, gk in zip(a, g):
            c = c + ak * gk
        S = c / np.float64(len(a) - 1)
        return np.float64(dn) * S


def impact_global(Xf, cap, weight):
    """(J, g): J_o per observation in input order from the members Xf at verification time, +0 where not USED, and
    g = dot(centered, weight)"""
    g = dot(Xf, weight, cap.t, True)[:, 0]
    M = len(g)
    J = np.zeros(len(cap.dn))
    used = cap.status == USED
    with np.errstate(all="ignore"):
        c = np.zeros(int(used.sum()))
        a = cap.a[used]
        for k in range(M):
            c = c + a[:, k] * g[k]
        J[used] = cap.dn[used] * (c / np.float64(M - 1))
    return J, g


def scale(cap, g):
    """sum_o sum_k |dn_o a_{o,k} g_k| / (M-1) over the USED observations: what the rounding of the total is relative to"""
    used = cap.status == USED
    return float(np.sum(np.abs(cap.dn[used, None] * cap.a[used] * g[None, :])) / (len(g) - 1))


summary = impact.summary


# ---- scenarios ---------------------------------------------------------------------------------------------------------
# shared by tests/test_gpu_impact_global.py and tools/impact_global_cpu_study.py, which ran them on the CPU first

GRID = (33, 17, 1.0, 1.0, 2.25)       # nx, ny, dx, dy, loc: the OSSE grid of tests/test_gpu_ensemble_impact.py
OSSE_B, OSSE_R, OSSE_STEPS = 21, 0.04, 6
COMMON_PHYS = (0.05, 0.1, 0.5, -0.25)  # D, dt, vx, vy of every member of the identity scenario
OSSE_PHYS = [(0.05, 0.1, 0.5, -0.25), (0.02, 0.1, -0.3, 0.4), (0.08, 0.05, 0.0, 0.0), (0.01, 0.1, 0.2, 0.2),
             (0.03, 0.1, -0.2, -0.1)]   # member m takes entry m % 5, as tests/test_gpu_ensemble_impact.py
IDENTITY_SIDES = [("pppp", 0.0), ("dddd", 0.5)]
IDENTITY_INFLATIONS = (1.0, 1.1)
SEEDS = range(1, 9)


def osse_members(seed):
    """osse_setup of tests/test_gpu_ensemble_impact.py for any seed: a smooth truth (member 0), twenty members around
    another smooth field, 40 stations on a lattice -> (X, i, j)"""
    nx, ny = GRID[:2]
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(ny + 2), np.arange(nx + 2), indexing="ij")

    def smooth():
        a = rng.standard_normal(4)
        return (a[0] * np.sin(2 * np.pi * ii / nx) + a[1] * np.cos(2 * np.pi * jj / ny)
                + a[2] * np.sin(2 * np.pi * (ii / nx + jj / ny)) + a[3] * np.cos(4 * np.pi * ii / nx)) / 2.0

    X = np.empty((OSSE_B, ny + 2, nx + 2))
    X[0] = smooth()
    base = X[0] + 0.4 * smooth()
    for m in range(1, OSSE_B):
        X[m] = base + 0.4 * smooth() + 0.02 * rng.standard_normal((ny + 2, nx + 2))
    I, J = np.meshgrid(np.arange(3, nx, 4), np.arange(3, ny, 3))
    return X, I.ravel().astype(np.int32), J.ravel().astype(np.int32)


def identity_members(seed, sides):
    """osse_members for the identity: a Periodic side keeps the ghosts it was given (the reference's Periodic is a no-op),
    so there the forecast is linear in the state only when the members share one ring: every member gets the truth's"""
    X, i, j = osse_members(seed)
    if "p" in sides:
        ring = np.ones(X.shape[1:], dtype=bool)
        ring[1:-1, 1:-1] = False
        X[:, ring] = X[0, ring]
    return X, i, j


def identity_values(X, i, j, seed):
    """the truth at the stations plus unbiased noise of variance OSSE_R, drawn on the host"""
    z = np.random.default_rng([seed, 77]).standard_normal(len(i))
    return X[0, j, i] + np.sqrt(OSSE_R) * z


def mse(mean, truth):
    return float(np.mean((mean[1:-1, 1:-1] - truth[1:-1, 1:-1]) ** 2))


def identity_figures(Xa, Xb, cap, weight_of):
    """from the forecasts Xa (after the analysis) and Xb (without it), truth member 0, and the capture:
    (total, actual, scale, gap / scale) of the identity  sum_o J_o = mse_a - mse_b"""
    mean_a, mean_b, truth = Xa[1:].mean(axis=0), Xb[1:].mean(axis=0), Xa[0]
    w = weight_of(mean_a, mean_b, truth)
    J, g = impact_global(Xa, cap, w)
    total = summary(J, cap.status)[2]
    ea, eb = mse(mean_a, truth), mse(mean_b, truth)
    sc = scale(cap, g) + ea + eb
    return total, ea - eb, sc, abs(total - (ea - eb)) / sc
