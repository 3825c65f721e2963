"""numpy restatements of the ETKF block of include/csim.h: the observation-space Gram matrix of csim_ensemble_obs_gram in
its stated order and the weights of csim_etkf_weights; an exact reference of the matrix and its derived bound; the dense
Kalman update that the weights are held against; and the helpers that tests/test_etkf_host.py and
tests/test_gpu_etkf.py share.

Every restatement does one rounded numpy operation per operation of the definition (numpy never contracts a * b + c),
so the GPU result can be compared bit for bit.  The eigensolver is the library's host-only sym_eigen, passed in."""
import math
from fractions import Fraction

import numpy as np

SEG = 64
MAX_MEMBERS = 256
U = 2.0 ** -53


def gram_plan(M, nobs):
    """(nseg, Gc) of csim_obs_gram_plan"""
    nseg = -(-nobs // SEG)
    cap = 1024 if M <= 64 else 256 if M <= 128 else 64
    return nseg, min(nseg, cap)


def plan_order(lev):
    """input indices in plan order, (level, input index), from the levels of ensemble_assim_plan"""
    return np.argsort(np.asarray(lev), kind="stable")


def rows(H, y, r, used, order):
    """(Z, E): Z (nobs, M + 1), the z_a of every plan position, and E (nobs, M), its e_k; +0 where not used.
    H: (M, nobs) operator values, y, r and used in input order"""
    H = np.asarray(H, dtype=np.float64)[:, order]
    M, n = H.shape
    y = np.asarray(y, dtype=np.float64)[order]
    sr = np.sqrt(np.broadcast_to(np.asarray(r, dtype=np.float64), (n,)))[order]
    used = np.broadcast_to(np.asarray(used, dtype=bool), (n,))[order]
    with np.errstate(all="ignore"):
        s = np.zeros(n)
        for k in range(M):
            s = s + H[k]
        hb = s / float(M)
        Z = np.empty((n, M + 1))
        Z[:, :M] = ((H - hb) / sr).T
        Z[:, M] = (y - hb) / sr
        E = ((y - H) / sr).T.copy()
    Z[~used] = 0.0
    E[~used] = 0.0
    return Z, E


def ordered_sums(Z, M, outer=True):
    """sum over the rows q of Z of z z^T (outer) or of z z (elementwise), in the order of csim_ensemble_obs_gram: class
    partials as running sums in increasing q, folded in class order starting from partial 0.  M decides the cap"""
    n, w = Z.shape
    nseg, Gc = gram_plan(M, n)
    shape = (w, w) if outer else (w,)
    acc = np.zeros((Gc,) + shape)
    term = np.empty((Gc,) + shape)
    with np.errstate(all="ignore"):
        for trip in range(-(-nseg // Gc)):
            for c in range(SEG):
                first = trip * Gc * SEG + c
                if first >= n:
                    break
                k = min(Gc, (n - 1 - first) // SEG + 1)
                v = Z[first:first + k * SEG:SEG]  # (k, w): class g's row c of this trip
                if outer:
                    np.multiply(v[:, :, None], v[:, None, :], out=term[:k])
                else:
                    np.multiply(v, v, out=term[:k])
                np.add(acc[:k], term[:k], out=acc[:k])
        out = acc[0]
        for g in range(1, Gc):
            out = out + acc[g]
    return out


def obs_gram(H, y, r, used, order, loglik=False):
    """(A, loglik or None, n_used) of csim_ensemble_obs_gram"""
    M = np.asarray(H).shape[0]
    Z, E = rows(H, y, r, used, order)
    A = ordered_sums(Z, M)
    ll = ordered_sums(E, M, outer=False) if loglik else None
    n = np.asarray(H).shape[1]
    return A, ll, int(np.count_nonzero(np.broadcast_to(np.asarray(used, dtype=bool), (n,))))


def class_rows(M, nobs):
    """the most plan positions that one class sums"""
    nseg, Gc = gram_plan(M, nobs)
    return max(sum(min(SEG, nobs - q * SEG) for q in range(g, nseg, Gc)) for g in range(Gc))


def gram_exact(Z):
    """the exact sum of z z^T over the rows of Z, as Fractions"""
    F = [[Fraction(float(v)) for v in row] for row in Z]
    w = Z.shape[1]
    return [[sum((row[a] * row[b] for row in F), Fraction(0)) for b in range(w)] for a in range(w)]


def gram_bound(Z, M):
    """gamma_k sum |z_a z_b| per entry, gamma_k = k u / (1 - k u): every product is rounded once, then goes through at
    most (rows of its class) additions of the class's running sum and Gc - 1 of the fold, so no term meets more than
    k = 1 + most rows of one class + (Gc - 1) roundings: sum_bound of tests/reduce_restatement.py with this k (Higham,
    Accuracy and Stability, 2nd ed., 4.2).  Derived, not tuned."""
    _, Gc = gram_plan(M, Z.shape[0])
    ku = (1 + class_rows(M, Z.shape[0]) + (Gc - 1)) * U
    A = np.abs(Z)
    w = Z.shape[1]
    return ku / (1.0 - ku) * np.array([[math.fsum((A[:, a] * A[:, b]).tolist()) for b in range(w)] for a in range(w)])


def etkf_weights(A, inflation, sym_eigen):
    """(W, wbar, gamma, dfs, sweeps) of csim_etkf_weights"""
    A = np.asarray(A, dtype=np.float64)
    M = A.shape[0] - 1
    rho = np.float64(inflation) * np.float64(inflation)
    kappa = np.float64(M - 1) / rho
    e = sym_eigen(np.ascontiguousarray(A[:M, :M]))
    lam, V = e.lambda_, e.V
    G = np.where(lam > 0, lam, 0.0)
    f = 1.0 / (kappa + G)
    g = np.sqrt(np.float64(M - 1) * f)
    u = np.zeros(M)
    for a in range(M):
        u = u + V[a, :] * A[a, M]
    fu = f * u
    wbar, S = np.zeros(M), np.zeros((M, M))
    dfs = np.float64(0.0)
    for r in range(M):
        wbar = wbar + V[:, r] * fu[r]
        S = S + (V[:, r] * g[r])[:, None] * V[:, r][None, :]
        dfs = dfs + G[r] * f[r]
    W = np.triu(S) + np.triu(S, 1).T
    return W, wbar, G, float(dfs), e.sweeps


# ---- the dense Kalman update in observation space --------------------------------------------------------------------

def kalman_obs_space(H, y, r, inflation):
    """(mean, cov) of H x after the Kalman update with rho Pb, rho = inflation^2, by np.linalg.solve"""
    M, n = H.shape
    hb = H.mean(axis=0)
    Y = (H - hb).T                                   # (nobs, M)
    P = (inflation * inflation) * (Y @ Y.T) / (M - 1)
    S = P + np.diag(r)
    return hb + P @ np.linalg.solve(S, y - hb), P - P @ np.linalg.solve(S, P)


def etkf_obs_space(H, W, wbar):
    """(mean, cov) of H x after transform(W, wbar)"""
    M = H.shape[0]
    hb = H.mean(axis=0)
    Y = (H - hb).T
    Ya = Y @ W
    return hb + Y @ wbar, Ya @ Ya.T / (M - 1)


def etkf_eigh(H, y, r, inflation):
    """(W, wbar) of a plain numpy ETKF on eigh, the yardstick of the Kalman check"""
    M = H.shape[0]
    hb = H.mean(axis=0)
    Z = ((H - hb) / np.sqrt(r)).T
    C, c = Z.T @ Z, Z.T @ ((y - hb) / np.sqrt(r))
    lam, V = np.linalg.eigh(C)
    lam = np.maximum(lam, 0.0)
    f = 1.0 / ((M - 1) / inflation ** 2 + lam)
    return (V * np.sqrt((M - 1) * f)) @ V.T, V @ (f * (V.T @ c))


def kalman_distance(H, y, r, inflation, W, wbar):
    """the larger of the relative max-norm distances of mean and covariance from the dense Kalman update"""
    m0, P0 = kalman_obs_space(H, y, r, inflation)
    m1, P1 = etkf_obs_space(H, W, wbar)
    return max(np.max(np.abs(m1 - m0)) / np.max(np.abs(m0)), np.max(np.abs(P1 - P0)) / np.max(np.abs(P0)))
