"""numpy restatement of the LETKF block of include/csim.h (csim_ensemble_assimilate_letkf), steps 2 to 5, written from
the header text: the lattice of analysis nodes, a cell's four nodes and weights, the Gram matrix of a node, the weights
of a node, and the cell pass.  On top of tests/local_analysis_restatement.py (L(c), the priors, the inflation) and
tests/etkf_restatement.py (the weights) by import only.  The eigensolver is passed in, as in tests/test_etkf_host.py:
the tests hand it the library's host-only sym_eigen(order="round_robin"), which tests/test_eigen_rr_host.py holds
against its own restatement.  Beside it the textbook: a dense LETKF of every cell on numpy.linalg.eigh, the yardstick
of the Kalman checks.
Every running sum is a loop in the stated order from +0, one rounded numpy operation per operation of the text."""
import collections

import numpy as np

import etkf_restatement as etkf
import local_analysis_restatement as local
import obsnet_restatement as obsnet

OK, IDLE, NONFINITE, NOT_CONVERGED = 0, 1, 2, 3
MAX_NODES, MAX_BYTES = 65535, 1 << 30
MAX_SWEEPS = 64

Info = collections.namedtuple("Info", "dfs count sweeps status")


# ---- step 2: the lattice ---------------------------------------------------------------------------------------------

def axis_nodes(n, s):
    """the cells of the nodes along an axis of n cells"""
    na = 1 if n == 1 else -(-(n - 1) // s) + 1
    return [min(1 + a * s, n) for a in range(na)]


def nodes(nx, ny, s):
    """(nax, nay, xi, yj) of csim_letkf_nodes"""
    xi, yj = axis_nodes(nx, s), axis_nodes(ny, s)
    return len(xi), len(yj), xi, yj


def axis_blend(i, s, at):
    """(a, t): the interval of cell i between the nodes at the cells `at`, and the weight of its upper node"""
    if len(at) < 2:
        return 0, np.float64(0.0)
    a = min((i - 1) // s, len(at) - 2)
    return a, np.float64(i - at[a]) / np.float64(at[a + 1] - at[a])


def blend(nx, ny, s, i, j):
    """(node[4], beta[4]) of csim_letkf_blend: a node that does not exist is its lower neighbour with beta = +0"""
    nax, nay, xi, yj = nodes(nx, ny, s)
    a, tx = axis_blend(i, s, xi)
    b, ty = axis_blend(j, s, yj)
    ax, ay = np.float64(1.0) - tx, np.float64(1.0) - ty
    a1, b1 = min(a + 1, nax - 1), min(b + 1, nay - 1)
    return [b * nax + a, b * nax + a1, b1 * nax + a, b1 * nax + a1], [ay * ax, ay * tx, ty * ax, ty * tx]


def plan_bytes(M, nn):
    """bytes of csim_letkf_plan: every array of the node storage starts at a multiple of 256 bytes"""
    work = 0 if M <= 96 else 2 * M * M
    at = 0
    for size in (8 * nn * (M + 1) ** 2, 8 * nn * work, 8 * nn * M * M, 8 * nn * M, 8 * nn * M * M, 8 * nn * M, 8 * nn,
                 8 * nn, 4 * nn, 4 * nn, 4 * nn):
        at = (at + size + 255) // 256 * 256
    return at


# ---- step 3: the Gram matrix of a node -------------------------------------------------------------------------------

def node_gram(H, y, obs, re):
    """A_g: H (nobs, M) the priors, obs and re the list L(g) with its r / rho; one running sum in the list's order"""
    M = H.shape[1]
    A = np.zeros((M + 1, M + 1))
    with np.errstate(all="ignore"):
        for o, q in zip(obs, re):
            sre = np.sqrt(np.float64(q))
            s = np.float64(0.0)
            for k in range(M):
                s = s + H[o, k]
            hb = s / np.float64(M)
            z = np.empty(M + 1)
            z[:M] = (H[o] - hb) / sre
            z[M] = (np.float64(y[o]) - hb) / sre
            A = A + z[:, None] * z[None, :]
    return A


# ---- step 4: the weights of a node -----------------------------------------------------------------------------------

def node_weights(A, count, sym_eigen):
    """(status, W, wbar, dfs, sweeps); W and wbar are None where they are not defined"""
    if count == 0:
        return IDLE, None, None, 0.0, 0
    if not np.isfinite(A).all():
        return NONFINITE, None, None, 0.0, 0
    W, wbar, _, dfs, sweeps = etkf.etkf_weights(A, 1.0, sym_eigen)
    return (NOT_CONVERGED if sweeps == MAX_SWEEPS else OK), W, wbar, dfs, sweeps


# ---- step 5: one cell ------------------------------------------------------------------------------------------------

def cell_update(x, beta, parts):
    """x: (M,) the cell's members; parts[n] = (status, W, wbar) of its four nodes -> the new members, or None when the
    cell is not written"""
    M = len(x)
    remaining = [n for n in range(4) if beta[n] != 0.0]
    if all(parts[n][0] in (IDLE, NONFINITE) for n in remaining):
        return None
    with np.errstate(all="ignore"):
        s = np.float64(0.0)
        for k in range(M):
            s = s + x[k]
        m = s / np.float64(M)
        p = x - m
        c = np.zeros(M)
        for n in remaining:
            status, W, wbar = parts[n]
            if status in (IDLE, NONFINITE):
                d, sr = np.float64(0.0), p
            else:
                d, sr = np.float64(0.0), np.zeros(M)
                for k in range(M):
                    d = d + p[k] * wbar[k]
                    sr = sr + p[k] * W[k]
            c = c + beta[n] * (d + sr)
        return m + c


# ---- the whole call ----------------------------------------------------------------------------------------------------

def analysis(X, rho, i, j, taps, y, r, lam, t, s, sym_eigen, status=None):
    """steps 1 (the inflation and the priors) to 5 of csim_ensemble_assimilate_letkf.  X: (B, ny+2, nx+2) -> (the
    analysed copy, Info with (nay, nax) arrays, the state after the inflation); status: the screening's bytes (None:
    every observation is used)"""
    X = local.inflate(X, lam, t)
    B, ny2, nx2 = X.shape
    nx, ny = nx2 - 2, ny2 - 2
    F = obsnet.forecast(B, t)
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (len(i),))
    H = local.priors(X, t, i, j, taps)
    nax, nay, xi, yj = nodes(nx, ny, s)
    parts = []
    info = Info(np.zeros((nay, nax)), np.zeros((nay, nax), dtype=np.int32), np.zeros((nay, nax), dtype=np.int32),
                np.zeros((nay, nax), dtype=np.int32))
    for b in range(nay):
        for a in range(nax):
            obs, re = local.local_list(xi[a], yj[b], rho, i, j, r, status)
            A = node_gram(H, y, obs, re)
            st, W, wbar, dfs, sweeps = node_weights(A, len(obs), sym_eigen)
            parts.append((st, W, wbar))
            info.dfs[b, a], info.count[b, a], info.sweeps[b, a], info.status[b, a] = dfs, len(obs), sweeps, st
    out = X.copy()
    for cj in range(1, ny + 1):
        for ci in range(1, nx + 1):
            node, beta = blend(nx, ny, s, ci, cj)
            new = cell_update(X[F, cj, ci], beta, [parts[n] for n in node])
            if new is not None:
                out[F, cj, ci] = new
    return out, info, X


# ---- the textbook ------------------------------------------------------------------------------------------------------

def eigh_weights(H, y, obs, re):
    """(W, wbar) of a plain numpy ETKF on eigh over the list of a node"""
    M = H.shape[1]
    Hl = H[obs]
    hb = Hl.mean(axis=1)
    sre = np.sqrt(np.asarray(re))
    Z = (Hl - hb[:, None]) / sre[:, None]
    c = Z.T @ ((np.asarray(y)[obs] - hb) / sre)
    lam, V = np.linalg.eigh(Z.T @ Z)
    lam = np.maximum(lam, 0.0)
    f = 1.0 / ((M - 1) + lam)
    return (V * np.sqrt((M - 1) * f)) @ V.T, V @ (f * (V.T @ c))


def eigh_analysis(X, rho, i, j, taps, y, r, lam, t, s):
    """the same analysis with the weights of every node from numpy.linalg.eigh and the cell pass in matrix products"""
    X = local.inflate(X, lam, t)
    B, ny2, nx2 = X.shape
    nx, ny = nx2 - 2, ny2 - 2
    F = obsnet.forecast(B, t)
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (len(i),))
    H = local.priors(X, t, i, j, taps)
    nax, nay, xi, yj = nodes(nx, ny, s)
    M = len(F)
    parts = []
    for b in range(nay):
        for a in range(nax):
            obs, re = local.local_list(xi[a], yj[b], rho, i, j, r)
            parts.append(eigh_weights(H, y, obs, re) if obs else (np.eye(M), np.zeros(M)))
    out = X.copy()
    for cj in range(1, ny + 1):
        for ci in range(1, nx + 1):
            node, beta = blend(nx, ny, s, ci, cj)
            x = X[F, cj, ci]
            m = x.mean()
            W = sum(bn * parts[n][0] for n, bn in zip(node, beta))
            wbar = sum(bn * parts[n][1] for n, bn in zip(node, beta))
            out[F, cj, ci] = m + (x - m) @ wbar + (x - m) @ W
    return out


def mean_var(X, t):
    """(mean, variance with ddof = 1) of the forecast members on the interior"""
    F = obsnet.forecast(X.shape[0], t)
    Z = X[F][:, 1:-1, 1:-1]
    return Z.mean(axis=0), Z.var(axis=0, ddof=1)


def distance(A, B, t):
    """the larger of the relative max-norm distances of mean and variance of two analyses"""
    ma, va = mean_var(A, t)
    mb, vb = mean_var(B, t)
    return max(np.max(np.abs(ma - mb)) / np.max(np.abs(mb)), np.max(np.abs(va - vb)) / np.max(np.abs(vb)))
