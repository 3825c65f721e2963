"""A second numpy restatement of the analysis block of include/csim.h (csim_ensemble_assimilate and the network forms),
vectorised over the observations of a level.  `restate` in tests/test_gpu_ensemble_assim.py and
obsop_restatement.analysis visit the observations one by one in Python, which is fine for 40 of them and useless for
70 000.  The plan guarantees that the observations of one level have disjoint windows and that none (nor any of its
taps) lies in another's window, so a level can be updated with array operations along the observation axis: every h_k is
read before anything of the level is written, then the cells at one window offset of all its observations are updated
together.  Each sum is still a running sum from +0 in member (or tap) order, a Python loop over k of vector operations,
every product rounded, so the bits are those of the serial restatements; tests/test_assim_level_restatement_host.py pins
that.  Half-widths up to lx = ly = 1 only."""
import numpy as np


def forecast(B, t):
    """the forecast members in order; t: the truth member, None or -1 for none"""
    return np.array([k for k in range(B) if t is None or k != t], dtype=np.intp)


def operator_h(X, F, i, j, taps=None):
    """h_k of the members F at the observations (i, j), shape (len(F), nobs): the cell itself for point observations;
    with taps = (start, di, dj, w) the running sum from +0 over the taps in tap order, every product rounded"""
    i, j = np.asarray(i, dtype=np.intp), np.asarray(j, dtype=np.intp)
    F = np.asarray(F, dtype=np.intp)[:, None]
    if taps is None:
        return X[F, j[None, :], i[None, :]]
    start, di, dj, w = (np.asarray(v) for v in taps)
    first, nt = start[:-1].astype(np.intp), np.diff(start)
    h = np.zeros((F.shape[0], len(i)))
    with np.errstate(all="ignore"):
        for s in range(int(nt.max()) if len(i) else 0):
            o = np.flatnonzero(nt > s)
            k = first[o] + s
            h[:, o] = h[:, o] + w[k][None, :] * X[F, (j[o] + dj[k])[None, :], (i[o] + di[k])[None, :]]
    return h


def mv(X, t, i, j, taps=None):
    """mean and variance of h_k over the forecast members per observation (mv of csim_ensemble_relax applied to h_k):
    what the networks record before and after an analysis"""
    H = operator_h(X, forecast(X.shape[0], t), i, j, taps)
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


def plan_order(lev):
    """input indices in plan order (level, then input index): entry q is the observation at plan position q"""
    return np.argsort(np.asarray(lev), kind="stable")


def analysis(csim, X, dx, dy, i, j, y, r, loc, lam, t, ordered, taps=None, used=None):
    """X: (B, ny+2, nx+2) -> the analysed copy, the prior hbar and p per observation in input order (NaN where `used` is
    false: those observations neither read nor write) and the number of levels.  Levels from csim.ensemble_assim_plan
    on all observations, the table from csim.ensemble_gc_table; the inflation comes first, on every interior cell"""
    X = X.copy()
    B, ny2, nx2 = X.shape
    nx, ny = nx2 - 2, ny2 - 2
    F = forecast(B, t)
    M = len(F)
    n = len(i)
    i, j = np.asarray(i, dtype=np.intp), np.asarray(j, dtype=np.intp)
    y = np.asarray(y, dtype=np.float64)
    r = np.array(np.broadcast_to(np.asarray(r, dtype=np.float64), (n,)))
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    ly, lx = (rho.shape[0] - 1) // 2, (rho.shape[1] - 1) // 2
    assert lx <= 1 and ly <= 1, "the level restatement supports half-widths up to 1"
    lev = np.asarray(csim.ensemble_assim_plan(i, j, lx, ly, ordered)) if n else np.zeros(0, dtype=np.int32)
    nlevels = int(lev.max()) + 1 if n else 0
    used = np.ones(n, dtype=bool) if used is None else np.asarray(used).astype(bool)
    if taps is not None:
        start, di, dj, w = (np.asarray(v) for v in taps)
    hbar_all, p_all = np.full(n, np.nan), np.full(n, np.nan)
    den, cden = float(M), float(M - 1)
    with np.errstate(all="ignore"):
        if lam != 1.0:
            lm1 = lam - 1.0
            s = np.zeros((ny, nx))
            for m in F:
                s = s + X[m, 1:-1, 1:-1]
            xbar = s / den
            for m in F:
                x = X[m, 1:-1, 1:-1].copy()
                X[m, 1:-1, 1:-1] = x + lm1 * (x - xbar)
        for L in range(nlevels):
            S = np.flatnonzero((lev == L) & used)
            if not len(S):
                continue
            io, jo = i[S], j[S]
            # what the plan guarantees: the clipped windows of a level share no cell (so no anchor, and no tap, which
            # lies within its own window, is in another observation's window)
            cells = np.concatenate([(jo + b) * nx2 + (io + a) for b in range(-ly, ly + 1) for a in range(-lx, lx + 1)])
            inside = np.concatenate([(io + a >= 1) & (io + a <= nx) & (jo + b >= 1) & (jo + b <= ny)
                                     for b in range(-ly, ly + 1) for a in range(-lx, lx + 1)])
            assert len(np.unique(cells[inside])) == np.count_nonzero(inside), f"level {L}: windows overlap"
            if taps is None:
                H = operator_h(X, F, io, jo)
            else:
                cnt = np.diff(start)[S]
                sub = np.concatenate(([0], np.cumsum(cnt)))
                pick = np.concatenate([np.arange(start[o], start[o + 1]) for o in S]) if len(S) else np.zeros(0, int)
                H = operator_h(X, F, io, jo, (sub, di[pick], dj[pick], w[pick]))
            s = np.zeros(len(S))
            for k in range(M):
                s = s + H[k]
            hbar = s / den
            hp = H - hbar[None, :]
            ss = np.zeros(len(S))
            for k in range(M):
                ss = ss + hp[k] * hp[k]
            p = ss / cden
            d = p + r[S]
            alpha = 1.0 / (1.0 + np.sqrt(r[S] / d))
            delta = y[S] - hbar
            hbar_all[S], p_all[S] = hbar, p
            for b in range(-ly, ly + 1):
                for a in range(-lx, lx + 1):
                    rw = rho[b + ly, a + lx]
                    if not rw > 0:
                        continue
                    ci, cj = io + a, jo + b
                    v = np.flatnonzero((ci >= 1) & (ci <= nx) & (cj >= 1) & (cj <= ny))
                    if not len(v):
                        continue
                    ci, cj = ci[v], cj[v]
                    Xw = X[F[:, None], cj[None, :], ci[None, :]]        # (M, cells), a copy
                    s = np.zeros(len(v))
                    for k in range(M):
                        s = s + Xw[k]
                    xbar = s / den
                    c = np.zeros(len(v))
                    for k in range(M):
                        c = c + (Xw[k] - xbar) * hp[k, v]
                    g = (rw * (c / cden)) / d[v]
                    beta = alpha[v] * g
                    gd = g * delta[v]
                    for k in range(M):
                        X[F[k], cj, ci] = Xw[k] + (gd - beta * hp[k, v])
    return X, hbar_all, p_all, nlevels
