"""numpy restatement of the forecast-impact block of include/csim.h (csim_obs_network_impact_capture,
csim_ensemble_obs_impact, csim_obs_impact_fold), written from the header text: the capture (a_{o,k}, dn_o), the terms of
a window's cells, the lane-and-butterfly fold, J_o and the summary.  On top of tests/obsnet_restatement.py (forecast
members, the chunked sum) and tests/obsop_restatement.py (h_k of a linear observation) by import only.
tests/test_ensemble_impact_host.py pins fold to the library bit for bit; tests/test_gpu_ensemble_impact.py uses the rest
as the reference of the kernels.  The localisation table is an argument: csim_ensemble_gc_table, which
tests/test_ensemble_assim_host.py pins."""
import collections

import numpy as np

import obsnet_restatement as obsnet
import obsop_restatement as obsop

USED = 0
Capture = collections.namedtuple("Capture", "a dn status t")
Capture.__doc__ = """a: (nobs, M) analysis perturbations in observation space; dn: (nobs,) normalised innovations; status:
(nobs,) bytes of the recorded analysis; t: the truth member or None"""


def h_members(X, t, i, j, taps=None):
    """h_k of every forecast member, shape (M, nobs): the cell's bits of a point observation, the tap sum of a linear one"""
    if taps is not None:
        return obsop.h_members(X, t, i, j, taps)
    return np.array([X[k, j, i] for k in obsnet.forecast(X.shape[0], t)])


def capture(X, t, i, j, taps, y, hb, r, status=None):
    """impact_capture on the members X (B, ny+2, nx+2): ha = sum h_k / M from +0 in member order, a = h_k - ha;
    dn = (y - hb) / r; status None: the analysis was not screened, every observation was used"""
    H = h_members(X, t, i, j, taps)
    M, n = H.shape
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (n,))
    with np.errstate(all="ignore"):
        s = np.zeros(n)
        for hk in H:
            s = s + hk
        ha = s / float(M)
        a = (H - ha).T.copy()
        dn = (np.asarray(y, dtype=np.float64) - hb) / r
    st = np.zeros(n, dtype=np.uint8) if status is None else np.asarray(status, dtype=np.uint8).copy()
    return Capture(a, dn, st, t)


def fold(u):
    """term e to lane e % 64; each lane sums its terms in increasing e from +0; then l[j] = l[j] + l[j ^ h] for
    h = 32 .. 1, all j at once; l[0]"""
    u = np.asarray(u, dtype=np.float64).ravel()
    lanes = np.zeros(64)
    with np.errstate(all="ignore"):
        for e0 in range(0, len(u), 64):
            row = u[e0:e0 + 64]
            lanes[:len(row)] = lanes[:len(row)] + row      # lanes past the end get no term
        j = np.arange(64)
        for h in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[j ^ h]
    return lanes[0]


def plain_sum(u):
    """a running sum from +0 in the order given: what fold is not"""
    return np.add.accumulate(np.concatenate(([0.0], np.asarray(u, dtype=np.float64).ravel())))[-1]


def window(rho, nx, ny, io, jo):
    """(i0, i1, j0, j1) of the analysis's window clipped to the interior, and the table's part over it"""
    ly, lx = (rho.shape[0] - 1) // 2, (rho.shape[1] - 1) // 2
    i0, i1, j0, j1 = max(1, io - lx), min(nx, io + lx), max(1, jo - ly), min(ny, jo + ly)
    return (i0, i1, j0, j1), rho[j0 - jo + ly:j1 - jo + ly + 1, i0 - io + lx:i1 - io + lx + 1]


def terms(Xf, cap, rho, io, jo, a, weight):
    """u_e of one observation's window, row-major: (rho (c / (M-1))) w where rho > 0, +0 elsewhere"""
    B, ny2, nx2 = Xf.shape
    F = obsnet.forecast(B, cap.t)
    M = len(F)
    (i0, i1, j0, j1), rw = window(rho, nx2 - 2, ny2 - 2, io, jo)
    xs = [Xf[m, j0:j1 + 1, i0:i1 + 1] for m in F]
    with np.errstate(all="ignore"):
        s = np.zeros(rw.shape)
        for x in xs:
            s = s + x
        xbar = s / float(M)
        c = np.zeros(rw.shape)
        for x, ak in zip(xs, a):
            c = c + (x - xbar) * ak
        u = (rw * (c / float(M - 1))) * weight[j0:j1 + 1, i0:i1 + 1]
    return np.where(rw > 0, u, 0.0).ravel()


def impact(Xf, cap, rho, i, j, weight):
    """J_o per observation in input order from the members Xf at verification time; +0 where not USED"""
    J = np.zeros(len(i))
    with np.errstate(all="ignore"):
        for o in range(len(i)):
            if cap.status[o] != USED:
                continue
            J[o] = cap.dn[o] * fold(terms(Xf, cap, rho, int(i[o]), int(j[o]), cap.a[o], weight))
    return J


def summary(J, status):
    """(used, beneficial, total): total by the 256-chunk rule of csim_obs_cycle"""
    return (int(np.count_nonzero(np.asarray(status) == USED)), int(np.count_nonzero(J < 0)), obsnet.chunked(J))


def impact_weight(mean_a, mean_b, truth):
    """((mean_a - truth) + (mean_b - truth)) / (nx ny) on the interior, 0 on the ghost ring"""
    w = np.zeros(truth.shape)
    n = float((truth.shape[0] - 2) * (truth.shape[1] - 2))
    inner = (slice(1, -1), slice(1, -1))
    w[inner] = ((mean_a[inner] - truth[inner]) + (mean_b[inner] - truth[inner])) / n
    return w
