"""numpy restatement of the local-analysis block of include/csim.h (csim_ensemble_assimilate_local), written from the
header text, one cell at a time: the local list of a cell, the serial update of the cell's members and of the private
priors of the observations still to come, and the whole call (inflation, priors from the inflated state, every interior
cell).  Beside it the textbook the block claims to equal in exact arithmetic: an LETKF of one cell on
numpy.linalg.eigh with R_loc = diag(r / rho).  On top of tests/obsnet_restatement.py and tests/obsop_restatement.py by
import only.  tests/test_local_analysis_host.py compares the two and pins csim_obs_local_count;
tests/test_gpu_ensemble_local.py uses `analysis` as the reference of the kernels, bit for bit.
Every sum over the members is a loop in member order from +0; where several targets are updated in one step the loop
runs over arrays with one element per target, so each element sees the scalar operations of the text in their order."""
import numpy as np

import obsnet_restatement as obsnet
import obsop_restatement as obsop

MAX_OBS, MAX_DOUBLES, MAX_PRIOR_DOUBLES = 64, 4096, 1 << 26
USED = 0


def local_count(nx, ny, i, j, lx, ly):
    """brute force: per interior cell, (ny, nx), the observations whose clipped window rectangle contains it"""
    count = np.zeros((ny, nx), dtype=np.int32)
    for io, jo in zip(i, j):
        i0, i1, j0, j1 = max(1, io - lx), min(nx, io + lx), max(1, jo - ly), min(ny, jo + ly)
        count[j0 - 1:j1, i0 - 1:i1] += 1
    return count


def local_list(ci, cj, rho, i, j, r, status=None):
    """L(c) and re = r_o / rho_o(c) of its observations: used, c inside the window, rho > 0, re finite; input order"""
    ly, lx = (rho.shape[0] - 1) // 2, (rho.shape[1] - 1) // 2
    obs, re = [], []
    with np.errstate(all="ignore"):
        for o in range(len(i)):
            if status is not None and status[o] != USED:
                continue
            a, b = ci - int(i[o]), cj - int(j[o])
            if abs(a) > lx or abs(b) > ly:
                continue
            w = rho[b + ly, a + lx]
            if not w > 0:
                continue
            q = np.float64(r[o]) / w
            if not np.isfinite(q):
                continue
            obs.append(o)
            re.append(q)
    return obs, re


def cell_update(z, W, y, re):
    """the loop of the block for one cell.  z: (M,) the cell's members; W: (L, M) the priors of its local observations
    in order (copied: they are private); y, re: (L,) -> the analysed z"""
    M = len(z)
    L = len(y)
    V = np.vstack([np.asarray(z, dtype=np.float64)[None, :], np.asarray(W, dtype=np.float64).reshape(L, M)])
    fM, fM1 = np.float64(M), np.float64(M - 1)
    with np.errstate(all="ignore"):
        for o in range(L):
            w = V[o + 1].copy()
            s = np.float64(0.0)
            for k in range(M):
                s = s + w[k]
            hbar = s / fM
            hp = w - hbar
            ss = np.float64(0.0)
            for k in range(M):
                ss = ss + hp[k] * hp[k]
            p = ss / fM1
            d = p + np.float64(re[o])
            alpha = np.float64(1.0) / (np.float64(1.0) + np.sqrt(np.float64(re[o]) / d))
            delta = np.float64(y[o]) - hbar
            rows = [0] + list(range(o + 2, L + 1))   # z, then every observation after o
            T = V[rows]
            sv = np.zeros(len(rows))
            for k in range(M):
                sv = sv + T[:, k]
            vbar = sv / fM
            c = np.zeros(len(rows))
            for k in range(M):
                c = c + (T[:, k] - vbar) * hp[k]
            g = (c / fM1) / d
            beta = alpha * g
            gd = g * delta
            V[rows] = T + (gd[:, None] - beta[:, None] * hp[None, :])
    return V[0]


def inflate(X, lam, t):
    """step 2 on a copy: x_k + (lam - 1) (x_k - xbar) on the interior of the forecast members"""
    X = X.copy()
    F = obsnet.forecast(X.shape[0], t)
    with np.errstate(all="ignore"):
        if lam != 1.0:
            lm1 = lam - 1.0
            s = np.zeros(X.shape[1:])[1:-1, 1:-1]
            for m in F:
                s = s + X[m, 1:-1, 1:-1]
            xbar = s / float(len(F))
            for m in F:
                x = X[m, 1:-1, 1:-1].copy()
                X[m, 1:-1, 1:-1] = x + lm1 * (x - xbar)
    return X


def priors(X, t, i, j, taps=None):
    """h_{o,k}, (nobs, M): the observed cell's bits, or the operator of a linear observation"""
    F = obsnet.forecast(X.shape[0], t)
    if taps is None:
        return X[F][:, np.asarray(j), np.asarray(i)].T.copy()
    return obsop.h_members(X, t, i, j, taps).T.copy()


def analysis(X, rho, i, j, taps, y, r, lam, t, status=None):
    """steps 2 to 4 of csim_ensemble_assimilate_local.  X: (B, ny+2, nx+2) -> the analysed copy; status: the bytes of
    step 1 (None: every observation is used)"""
    X = inflate(X, lam, t)
    B, ny2, nx2 = X.shape
    F = obsnet.forecast(B, t)
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (len(i),))
    H = priors(X, t, i, j, taps)
    ly, lx = (rho.shape[0] - 1) // 2, (rho.shape[1] - 1) // 2
    # the cells that some window reaches at all; the others have an empty list
    near = np.zeros((ny2, nx2), dtype=bool)
    for io, jo in zip(i, j):
        near[max(1, jo - ly):min(ny2 - 2, jo + ly) + 1, max(1, io - lx):min(nx2 - 2, io + lx) + 1] = True
    out = X.copy()
    for cj, ci in zip(*np.nonzero(near)):
        obs, re = local_list(int(ci), int(cj), rho, i, j, r, status)
        if obs:
            out[F, cj, ci] = cell_update(X[F, cj, ci], H[obs], np.asarray(y, dtype=np.float64)[obs], re)
    return out


def touched(shape, rho, i, j, r, status=None):
    """interior cells with a non-empty list"""
    out = np.zeros(shape, dtype=bool)
    for cj in range(1, shape[0] - 1):
        for ci in range(1, shape[1] - 1):
            out[cj, ci] = bool(local_list(ci, cj, rho, i, j, r, status)[0])
    return out


def letkf_cell(z, W, y, re):
    """the LETKF of Hunt et al. 2007 for one cell with R_loc = diag(re), through a symmetric eigendecomposition in
    ensemble space: (analysis mean, analysis variance with ddof = 1) of the cell"""
    z, W = np.asarray(z, dtype=np.float64), np.asarray(W, dtype=np.float64)
    M = len(z)
    zbar = z.mean()
    zp = z - zbar
    ybar = W.mean(axis=1)
    Y = W - ybar[:, None]                      # (L, M)
    C = (Y / np.asarray(re)[:, None]).T        # Y^T R^-1, (M, L)
    lam, Q = np.linalg.eigh(C @ Y)
    Pa = (Q / ((M - 1) + lam)) @ Q.T           # [(M-1) I + Y^T R^-1 Y]^-1
    wbar = Pa @ (C @ (np.asarray(y) - ybar))
    return zbar + zp @ wbar, zp @ Pa @ zp      # var = z' [(M-1) Pa] z'^T / (M-1)
