"""numpy restatement of the linear-observation block of include/csim.h (csim_obs_network_create_linear and the two tap
builders), written from the header text: the operator h = sum_s w_s x(anchor + tap s), the serial filter with that
operator, observe, the diagnostics, and the builders.  On top of tests/obsnet_restatement.py (noise, mv's order, the
chunked sums of a csim_obs_cycle) and tests/perturb_restatement.py below it.  tests/test_ensemble_obsop_host.py pins the
builders to the library bit for bit; tests/test_gpu_ensemble_obsop.py uses the rest as the reference of the kernels.
The localisation table and the levels are arguments: they are csim_ensemble_gc_table and csim_ensemble_assim_plan on the
anchors, which tests/test_ensemble_assim_host.py pins."""
import math

import numpy as np

import obsnet_restatement as obsnet

MAX_TAPS = 64


def operator(x, i, j, taps):
    """x: one member (ny+2, nx+2) -> h per observation: every product rounded, a running sum from +0 in tap order"""
    start, di, dj, w = taps
    h = np.zeros(len(i))
    with np.errstate(all="ignore"):
        for o in range(len(i)):
            acc = np.float64(0.0)
            for s in range(int(start[o]), int(start[o + 1])):
                acc = acc + np.float64(w[s]) * x[int(j[o]) + int(dj[s]), int(i[o]) + int(di[s])]
            h[o] = acc
    return h


def h_members(X, t, i, j, taps):
    """h_k of every forecast member, shape (M, nobs)"""
    return np.array([operator(X[k], i, j, taps) for k in obsnet.forecast(X.shape[0], t)])


def mv(X, t, i, j, taps):
    """mv of csim_ensemble_relax applied to h_k over the forecast members, per observation"""
    H = h_members(X, t, i, j, taps)
    M = float(H.shape[0])
    with np.errstate(all="ignore"):
        s = np.zeros(H.shape[1])
        for hk in H:
            s = s + hk
        m = s / M
        q = np.zeros(H.shape[1])
        for hk in H:
            d = hk - m
            q = q + d * d
        return m, q / (M - 1.0)


def observe(X, s, i, j, taps, r, seed, draw, with_noise):
    """y, xt in input order: xt = h of member s; y = xt + sqrt(r) z (the product rounded, then the sum) or xt"""
    xt = operator(X[s], i, j, taps)
    if not with_noise:
        return xt.copy(), xt
    z = obsnet.noise(seed, draw, np.arange(len(i)))
    return xt + np.sqrt(np.broadcast_to(np.asarray(r, dtype=np.float64), xt.shape)) * z, xt


def analysis(X, rho, lev, i, j, taps, y, r, lam, t):
    """the serial filter of csim_ensemble_assimilate with h_k from the operator, windows centred on the anchors, in the
    order (level, input index).  X: (B, ny+2, nx+2) -> the analysed copy"""
    X = X.copy()
    B, ny2, nx2 = X.shape
    nx, ny = nx2 - 2, ny2 - 2
    F = obsnet.forecast(B, t)
    M = len(F)
    ly, lx = (rho.shape[0] - 1) // 2, (rho.shape[1] - 1) // 2
    start, di, dj, w = taps
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (len(i),))
    with np.errstate(all="ignore"):
        if lam != 1.0:
            lm1 = lam - 1.0
            s = np.zeros((ny, nx))
            for m in F:
                s = s + X[m, 1:-1, 1:-1]
            xbar = s / float(M)
            for m in F:
                x = X[m, 1:-1, 1:-1].copy()
                X[m, 1:-1, 1:-1] = x + lm1 * (x - xbar)
        for o in np.argsort(lev, kind="stable"):
            io, jo = int(i[o]), int(j[o])
            acc = np.zeros(M)                # all members at once: the same products and sums, element by element
            for s in range(int(start[o]), int(start[o + 1])):
                acc = acc + np.float64(w[s]) * X[F, jo + int(dj[s]), io + int(di[s])]
            h = list(acc)
            s = np.float64(0.0)
            for v in h:
                s = s + v
            hbar = s / float(M)
            hp = [v - hbar for v in h]
            ss = np.float64(0.0)
            for v in hp:
                ss = ss + v * v
            p = ss / float(M - 1)
            d = p + r[o]
            alpha = 1.0 / (1.0 + np.sqrt(r[o] / d))
            delta = y[o] - hbar
            i0, i1, j0, j1 = max(1, io - lx), min(nx, io + lx), max(1, jo - ly), min(ny, jo + ly)
            rw = rho[j0 - jo + ly:j1 - jo + ly + 1, i0 - io + lx:i1 - io + lx + 1]
            mask = rw > 0
            xs = [X[m, j0:j1 + 1, i0:i1 + 1] for m in F]  # views
            s = np.zeros(rw.shape)
            for x in xs:
                s = s + x
            xbar = s / float(M)
            c = np.zeros(rw.shape)
            for x, hk in zip(xs, hp):
                c = c + (x - xbar) * hk
            g = (rw * (c / float(M - 1))) / d
            beta = alpha * g
            for x, hk in zip(xs, hp):
                new = x + (g * delta - beta * hk)
                x[mask] = new[mask]
    return X


def windows(shape, rho, i, j):
    """interior cells inside some anchor's window with rho > 0"""
    ny2, nx2 = shape
    ly, lx = (rho.shape[0] - 1) // 2, (rho.shape[1] - 1) // 2
    out = np.zeros(shape, dtype=bool)
    for io, jo in zip(i, j):
        for b in range(-ly, ly + 1):
            for a in range(-lx, lx + 1):
                ci, cj = io + a, jo + b
                if 1 <= ci <= nx2 - 2 and 1 <= cj <= ny2 - 2 and rho[b + ly, a + lx] > 0:
                    out[cj, ci] = True
    return out


# ---- the builders -------------------------------------------------------------------------------------------------

def bilinear(nx, ny, x, y):
    """(i, j, di[4], dj[4], w[4]) for one position"""
    x, y = np.float64(x), np.float64(y)
    i = max(min(int(math.floor(x)), nx - 1), 1)
    j = max(min(int(math.floor(y)), ny - 1), 1)
    fx, fy = x - np.float64(i), y - np.float64(j)
    gx, gy = np.float64(1.0) - fx, np.float64(1.0) - fy
    ex, ey = (0 if nx == 1 else 1), (0 if ny == 1 else 1)
    return i, j, [0, ex, 0, ex], [0, 0, ey, ey], [gx * gy, fx * gy, gx * fy, fx * fy]


def box(nx, ny, i, j, a, b):
    """(di, dj, w) of the clipped box mean, or None above MAX_TAPS taps"""
    cells = [(u, v) for v in range(-b, b + 1) for u in range(-a, a + 1) if 1 <= i + u <= nx and 1 <= j + v <= ny]
    if len(cells) > MAX_TAPS:
        return None
    each = np.float64(1.0) / np.float64(len(cells))
    return [u for u, _ in cells], [v for _, v in cells], [each] * len(cells)


def concat(per_obs):
    """[(di, dj, w), ...] -> (start, di, dj, w) arrays"""
    start = np.concatenate(([0], np.cumsum([len(t[2]) for t in per_obs]))).astype(np.int32)
    cat = lambda k, dt: np.array([v for t in per_obs for v in t[k]], dtype=dt)
    return start, cat(0, np.int32), cat(1, np.int32), cat(2, np.float64)


def check(nx, ny, lx, ly, i, j, taps):
    """the constraints of csim_obs_linear_check: True when all hold"""
    start, di, dj, w = taps
    n = len(i)
    if n < 1 or len(start) != n + 1 or start[0] != 0:
        return False
    for o in range(n):
        nt = start[o + 1] - start[o]
        if nt < 1 or nt > MAX_TAPS:
            return False
    for o in range(n):
        if not (1 <= i[o] <= nx and 1 <= j[o] <= ny):
            return False
        for s in range(start[o], start[o + 1]):
            if not (1 <= i[o] + di[s] <= nx and 1 <= j[o] + dj[s] <= ny):
                return False
            if abs(di[s]) > lx or abs(dj[s]) > ly or not np.isfinite(w[s]):
                return False
    return True
