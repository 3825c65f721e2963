"""numpy restatement of the round-robin Jacobi order of include/csim.h (CSIM_EIGEN_ROUND_ROBIN), written the way the
header defines a step and the device kernel computes it: the parameters of every slot from the matrix as it stands at
the start of the step, then every 2 x 2 block of two slots K < L rotated as rows by K and as columns by L.  The library's
host code takes the slots one after the other instead; the two must agree bit for bit.  Every numpy operation below is
one IEEE fp64 operation on whole arrays: no FMA, no reordering."""
import numpy as np

MAX_SWEEPS = 64


def pairs(n, t):
    """the slots of step t: arrays p < q of length m / 2, m = n rounded up to even; q >= n marks an idle slot"""
    m = n + (n & 1)
    k = np.arange(1, m // 2)
    x = np.concatenate([[m - 1], (t + k) % (m - 1)])
    y = np.concatenate([[t], (t - k) % (m - 1)])
    return np.minimum(x, y), np.maximum(x, y)


def slot_parameters(a, p, q):
    """(on, s, tau) per slot, and the slot's own three entries of a updated in place"""
    n = a.shape[0]
    S = len(p)
    on = np.zeros(S, dtype=bool)
    s, tau = np.zeros(S), np.zeros(S)
    for k in range(S):
        if q[k] >= n:
            continue
        pp, qq = int(p[k]), int(q[k])
        apq = a[pp, qq]
        if apq == 0.0:
            continue
        g = np.abs(apq)
        app, aqq = a[pp, pp], a[qq, qq]
        if np.abs(app) + g == np.abs(app) and np.abs(aqq) + g == np.abs(aqq):
            a[pp, qq] = a[qq, pp] = 0.0
            continue
        h = aqq - app
        if np.abs(h) + g == np.abs(h):
            t = apq / h
        else:
            theta = (np.float64(0.5) * h) / apq
            t = np.float64(1.0) / (np.abs(theta) + np.sqrt(theta * theta + np.float64(1.0)))
            if theta < 0.0:
                t = -t
        c = np.float64(1.0) / np.sqrt(t * t + np.float64(1.0))
        s[k] = t * c
        tau[k] = s[k] / (np.float64(1.0) + c)
        h = t * apq
        a[pp, pp] = app - h
        a[qq, qq] = aqq + h
        a[pp, qq] = a[qq, pp] = 0.0
        on[k] = True
    return on, s, tau


def rot(x, y, s, tau, on):
    xn = x - s * (y + x * tau)
    yn = y + s * (x - y * tau)
    return np.where(on, xn, x), np.where(on, yn, y)


def step(a, v, t):
    """one step of a sweep on a (n x n, symmetric) and v (row p is vector p), in place"""
    n = a.shape[0]
    p, q = pairs(n, t)
    S = len(p)
    on, s, tau = slot_parameters(a, p, q)
    K, L = np.triu_indices(S, 1)
    if len(K):
        # an idle slot's q is out of range: it reads a dummy row / column of zeros and stores nothing there
        pad = np.zeros((n + 1, n + 1))
        pad[:n, :n] = a
        pK, qK, pL, qL = p[K], np.minimum(q[K], n), p[L], np.minimum(q[L], n)
        x00, x01, x10, x11 = pad[pK, pL], pad[pK, qL], pad[qK, pL], pad[qK, qL]
        x00, x10 = rot(x00, x10, s[K], tau[K], on[K])   # rows, by K: x, y are the two entries of a column
        x01, x11 = rot(x01, x11, s[K], tau[K], on[K])
        x00, x01 = rot(x00, x01, s[L], tau[L], on[L])   # then columns, by L
        x10, x11 = rot(x10, x11, s[L], tau[L], on[L])
        for i, j, x in ((pK, pL, x00), (pK, qL, x01), (qK, pL, x10), (qK, qL, x11)):
            pad[i, j] = x
            pad[j, i] = x
        a[:, :] = pad[:n, :n]
    for k in np.nonzero(on)[0]:
        x, y = v[p[k]].copy(), v[q[k]].copy()
        v[p[k]], v[q[k]] = rot(x, y, s[k], tau[k], True)


def sym_eigen_rr(A, after_step=None):
    """(lambda, V, sweeps) of the upper triangle of A; after_step(a) is called with the working matrix after every step"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    a = np.triu(A) + np.triu(A, 1).T
    v = np.eye(n)
    m = n + (n & 1)
    done = 0
    while done < MAX_SWEEPS:
        if not np.triu(a, 1).any():
            break
        for t in range(m - 1):
            step(a, v, t)
            if after_step:
                after_step(a)
        done += 1
    d = np.diag(a).copy()
    order = sorted(range(n), key=lambda i: (-d[i], i)) if not np.isnan(d).any() else list(range(n))
    lam = d[order]
    V = np.empty((n, n))
    for r, src in enumerate(order):
        big = int(np.argmax(np.abs(v[src])))  # the first of equal magnitudes
        V[:, r] = -v[src] if v[src, big] < 0.0 else v[src]
    return lam, V, done
