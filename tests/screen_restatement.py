"""numpy restatement of the screening block of include/csim.h (csim_obs_network_set_active,
csim_ensemble_assimilate_screened), written from the header text: the decision of one observation, the statuses of a
network, the csim_obs_cycle of a screened analysis (terms of observations that are not used are +0, n the number used)
and the csim_obs_screen_cycle beside it.  On top of tests/obsnet_restatement.py and tests/obsop_restatement.py by import
only.  tests/test_ensemble_screen_host.py pins decide to the library bit for bit; tests/test_gpu_ensemble_screen.py uses
the rest as the reference of the kernels.  The analysis oracle for ordered = 0 is obsop_restatement.analysis with the
USED subset and the full plan's levels restricted to it (subset_analysis)."""
import numpy as np

import obsnet_restatement as obsnet
import obsop_restatement as obsop

USED, INACTIVE, REJECTED = 0, 1, 2
SCREEN_FIELDS = ("n_used", "n_inactive", "n_rejected")


def decide(y, hb, vb, r, tol, active=True):
    """steps 2 and 3 for one observation: the mask wins and y is not looked at; k2 = tol * tol rounded;
    REJECTED iff tol > 0 and not (t t <= k2 (vb + r)), every product rounded"""
    if not active:
        return INACTIVE
    tol = np.float64(tol)
    if not tol > 0:
        return USED
    with np.errstate(all="ignore"):
        k2 = tol * tol
        t = np.float64(y) - np.float64(hb)
        lhs = t * t
        rhs = k2 * (np.float64(vb) + np.float64(r))
    return USED if lhs <= rhs else REJECTED


def statuses(y, hb, vb, r, tol, active=None):
    """the status byte of every observation, input order"""
    n = len(y)
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (n,))
    active = np.ones(n, dtype=bool) if active is None else np.asarray(active).astype(bool)
    tol = np.float64(tol)
    st = np.zeros(n, dtype=np.uint8)
    if tol > 0:
        with np.errstate(all="ignore"):
            k2 = tol * tol
            t = np.asarray(y, dtype=np.float64) - hb
            lhs = t * t
            rhs = k2 * (np.asarray(vb, dtype=np.float64) + r)
            st[~(lhs <= rhs)] = REJECTED
    st[~active] = INACTIVE
    return st


def cycle(y, hb, vb, ha, va, r, status, xt=None):
    """the csim_obs_cycle of a screened, recorded analysis: every term of an observation that is not USED is +0"""
    n = len(y)
    used = np.asarray(status) == USED
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (n,))
    z = lambda terms: np.where(used, terms, 0.0)
    with np.errstate(all="ignore"):
        ob, oa, ab = y - hb, y - ha, ha - hb
        rec = dict(n=float(np.count_nonzero(used)), has_truth=0.0 if xt is None else 1.0,
                   sum_ob=obsnet.chunked(z(ob)), sum_ob2=obsnet.chunked(z(ob * ob)), sum_oa=obsnet.chunked(z(oa)),
                   sum_oa2=obsnet.chunked(z(oa * oa)), sum_oa_ob=obsnet.chunked(z(oa * ob)),
                   sum_ab_ob=obsnet.chunked(z(ab * ob)), sum_vb=obsnet.chunked(z(vb)), sum_va=obsnet.chunked(z(va)),
                   sum_r=obsnet.chunked(z(r)), sum_eb2=np.float64(0.0), sum_ea2=np.float64(0.0))
        if xt is not None:
            eb, ea = hb - xt, ha - xt
            rec["sum_eb2"], rec["sum_ea2"] = obsnet.chunked(z(eb * eb)), obsnet.chunked(z(ea * ea))
    return rec


def screen_cycle(status):
    status = np.asarray(status)
    return dict(n_used=float(np.count_nonzero(status == USED)), n_inactive=float(np.count_nonzero(status == INACTIVE)),
                n_rejected=float(np.count_nonzero(status == REJECTED)))


def subset_analysis(X, rho, lev, i, j, taps, y, r, lam, t, status):
    """step 4: the inflation on every interior cell, then the serial filter over the USED observations in the order
    (level, input index) of the full plan.  taps = (start, di, dj, w) of all observations"""
    keep = np.flatnonzero(np.asarray(status) == USED)
    start, di, dj, w = taps
    per = [(list(di[start[o]:start[o + 1]]), list(dj[start[o]:start[o + 1]]), list(w[start[o]:start[o + 1]]))
           for o in keep]
    sub = obsop.concat(per) if len(keep) else (np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32),
                                               np.zeros(0, dtype=np.int32), np.zeros(0))
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (len(i),))
    return obsop.analysis(X, rho, np.asarray(lev)[keep], np.asarray(i)[keep], np.asarray(j)[keep], sub,
                          np.asarray(y)[keep], r[keep], lam, t)


def point_taps(n):
    """the one-tap (0, 0, 1.0) operator of n point observations (equal to them bit for bit where no -0 is in play)"""
    return (np.arange(n + 1, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.ones(n))
