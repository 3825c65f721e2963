"""The relaxation inflation of include/csim.h (csim_ensemble_prior_capture / csim_ensemble_relax) restated in numpy:
every sum a running sum from +0 over the forecast members in their order (the member loops are explicit), every
operation one IEEE fp64 operation (numpy neither reorders nor fuses), / and sqrt correctly rounded.  Fields are in the
reference layout, (B, ny + 2, nx + 2); only the interior of the forecast members is read or written."""
import numpy as np

SPREAD, PERT = 1, 2


def forecast(B, t):
    """indices of the forecast members: all B, or the B - 1 others with truth member t"""
    return [k for k in range(B) if t is None or k != t]


def mean(x):
    """m of mv(x); x: (M, ...)"""
    s = np.zeros(x.shape[1:])
    for k in range(x.shape[0]):
        s = s + x[k]
    return s / float(x.shape[0])


def mv(x):
    """(m, v) of mv(x); x: (M, ...)"""
    M = x.shape[0]
    m = mean(x)
    q = np.zeros(x.shape[1:])
    for k in range(M):
        d = x[k] - m
        q = q + d * d
    return m, q / float(M - 1)


def capture(X, mode, t=None):
    """what a capture keeps of the state X: sb of the interior (SPREAD) or the interiors of the forecast members (PERT)"""
    with np.errstate(all="ignore"):
        x = X[forecast(X.shape[0], t)][:, 1:-1, 1:-1]
        if mode == SPREAD:
            return np.sqrt(mv(x)[1])
        return x.copy()


def relax(X, cap, mode, alpha, t=None):
    """the state after csim_ensemble_relax and, for SPREAD, the factor field (ny + 2, nx + 2) with its ring of +0"""
    out = np.array(X, dtype=np.float64, copy=True)
    if alpha == 0.0:
        return out, (np.zeros(X.shape[1:]) if mode == SPREAD else None)
    ks = forecast(X.shape[0], t)
    with np.errstate(all="ignore"):
        x = X[ks][:, 1:-1, 1:-1]
        if mode == SPREAD:
            m, v = mv(x)
            sa = np.sqrt(v)
            f = np.where(sa > 0, alpha * ((cap - sa) / sa), 0.0)
            write = ~(f == 0)
            for n, k in enumerate(ks):
                new = x[n] + f * (x[n] - m)
                out[k, 1:-1, 1:-1] = np.where(write, new, x[n])
            factor = np.zeros(X.shape[1:])
            factor[1:-1, 1:-1] = f
            return out, factor
        m, mb = mean(x), mean(cap)
        for n, k in enumerate(ks):
            out[k, 1:-1, 1:-1] = x[n] + alpha * ((cap[n] - mb) - (x[n] - m))
        return out, None
