"""numpy restatement of the observation-network block of include/csim.h (csim_obs_network_*), written from the text:
the observation noise on top of the Philox and normal-quantile restatement of tests/perturb_restatement.py, observe,
the per-observation mean and variance over the forecast members, and the chunked sums of a csim_obs_cycle.
tests/test_ensemble_obsnet_host.py pins the noise to the library bit for bit and the sums to closed forms;
tests/test_gpu_ensemble_obsnet.py uses the rest as the reference of the kernels."""
import numpy as np

import perturb_restatement as pr

CHUNK = 256
FIELDS = ("n", "has_truth", "sum_ob", "sum_ob2", "sum_oa", "sum_oa2", "sum_oa_ob", "sum_ab_ob", "sum_vb", "sum_va",
          "sum_r", "sum_eb2", "sum_ea2")


def noise(seed, draw, o):
    """z_o for an array of input indices: the first 64 bits of philox(ctr = (o, 0, 0xFFFFFFFF, draw), key = seed)"""
    o = np.atleast_1d(np.asarray(o, dtype=np.uint64))
    out = pr.philox([o, np.zeros_like(o), np.full_like(o, 0xFFFFFFFF), np.full_like(o, draw)],
                    [seed & 0xFFFFFFFF, seed >> 32])
    return pr.normal_from_bits(out[0] | (out[1] << pr.S32)).reshape(o.shape)


def observe(X, s, i, j, r, seed, draw, with_noise):
    """X: (B, ny+2, nx+2) -> y, xt in input order"""
    xt = X[s, j, i].copy()
    if not with_noise:
        return xt.copy(), xt
    z = noise(seed, draw, np.arange(len(i)))
    return xt + np.sqrt(np.asarray(r, dtype=np.float64)) * z, xt


def forecast(B, t):
    return [k for k in range(B) if k != t]


def mv(X, t, i, j):
    """mean and variance over the forecast members at each observation's cell: running sums from +0 in member order"""
    ks = forecast(X.shape[0], t)
    M = float(len(ks))
    with np.errstate(all="ignore"):
        s = np.zeros(len(i))
        for k in ks:
            s = s + X[k, j, i]
        m = s / M
        q = np.zeros(len(i))
        for k in ks:
            d = X[k, j, i] - m
            q = q + d * d
        return m, q / (M - 1.0)


def chunked(terms):
    """T_c: the running sum from +0 over each chunk of 256 consecutive terms; then the running sum of T_c from +0"""
    terms = np.asarray(terms, dtype=np.float64)
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for c in range(0, len(terms), CHUNK):
            T = np.add.accumulate(np.concatenate(([0.0], terms[c:c + CHUNK])))[-1]  # accumulate is strictly serial
            total = total + T
    return total


def cycle(y, hb, vb, ha, va, r, xt=None):
    """the csim_obs_cycle of one recorded analysis, as a dict"""
    n = len(y)
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (n,))
    with np.errstate(all="ignore"):
        ob, oa, ab = y - hb, y - ha, ha - hb
        rec = dict(n=float(n), has_truth=0.0 if xt is None else 1.0, sum_ob=chunked(ob), sum_ob2=chunked(ob * ob),
                   sum_oa=chunked(oa), sum_oa2=chunked(oa * oa), sum_oa_ob=chunked(oa * ob),
                   sum_ab_ob=chunked(ab * ob), sum_vb=chunked(vb), sum_va=chunked(va), sum_r=chunked(r),
                   sum_eb2=np.float64(0.0), sum_ea2=np.float64(0.0))
        if xt is not None:
            eb, ea = hb - xt, ha - xt
            rec["sum_eb2"], rec["sum_ea2"] = chunked(eb * eb), chunked(ea * ea)
    return rec
