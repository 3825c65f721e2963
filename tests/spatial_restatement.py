"""numpy / plain-Python restatement of the neighbourhood and probability verification (csim_ensemble_verify_spatial and
csim_verify_spatial_finish of include/csim.h), shared by the host and the GPU tests.  The integer half (counts, truth
bits, contingency table, window sums) is exact; the finishing repeats the header's formulas in the header's order with
Python floats (IEEE double, one rounding per operation), so the C function must agree bit for bit."""
import math

import numpy as np

NAN = float("nan")


def counts(members, truth, thresholds):
    """members (M, ny+2, nx+2), truth (ny+2, nx+2) -> n (nt, ny, nx), o (nt, ny, nx) int64 and the NaN mask (ny, nx):
    the interior only, strict comparisons, both 0 on a NaN cell"""
    x = np.asarray(members, dtype=np.float64)[:, 1:-1, 1:-1]
    y = np.asarray(truth, dtype=np.float64)[1:-1, 1:-1]
    nan = np.isnan(y) | np.isnan(x).any(axis=0)
    with np.errstate(invalid="ignore"):
        n = np.stack([(x > t).sum(axis=0) for t in thresholds]).astype(np.int64)
        o = np.stack([(y > t) for t in thresholds]).astype(np.int64)
    n[:, nan] = 0
    o[:, nan] = 0
    return n, o, nan


def window_sums(a, half):
    """sum of a (ny, nx) int64 over the (2 half + 1)^2 window centred on each cell, zero outside: padded 2-D cumulative
    sums in int64"""
    ny, nx = a.shape
    p = np.zeros((ny + 2 * half + 1, nx + 2 * half + 1), dtype=np.int64)
    p[half + 1:half + 1 + ny, half + 1:half + 1 + nx] = a
    # a[j, i] sits at p[j + half + 1, i + half + 1] behind a zero first row and column, so with s the inclusive sums
    # the window of (j, i), rows j - half .. j + half of a, is s[j + w, i + w] - s[j, i + w] - s[j + w, i] + s[j, i]
    s = p.cumsum(axis=0).cumsum(axis=1)
    w = 2 * half + 1
    return s[w:w + ny, w:w + nx] - s[0:ny, w:w + nx] - s[w:w + ny, 0:nx] + s[0:ny, 0:nx]


def window_sums_brute(a, half):
    ny, nx = a.shape
    out = np.zeros((ny, nx), dtype=np.int64)
    for j in range(ny):
        for i in range(nx):
            for dj in range(-half, half + 1):
                for di in range(-half, half + 1):
                    jj, ii = j + dj, i + di
                    if 0 <= jj < ny and 0 <= ii < nx:
                        out[j, i] += a[jj, ii]
    return out


def tables(n, o, nan, M, halves, window=window_sums):
    """the integer outputs: table (nt, M+1, 2) and nbh (nt, ns, 3) uint64, cells, nan_cells"""
    nt = n.shape[0]
    ok = ~nan
    table = np.zeros((nt, M + 1, 2), dtype=np.uint64)
    nbh = np.zeros((nt, len(halves), 3), dtype=np.uint64)
    for q in range(nt):
        for b in (0, 1):
            table[q, :, b] = np.bincount(n[q][ok & (o[q] == b)], minlength=M + 1).astype(np.uint64)
        for s, h in enumerate(halves):
            F, O = window(n[q], h), window(o[q], h)
            for c, v in enumerate((F * F, O * O, F * O)):
                nbh[q, s, c] = int(v[ok].sum(dtype=np.int64))
    return table, nbh, int(ok.sum()), int(nan.sum())


def restate(members, truth, thresholds, halves, M=None):
    n, o, nan = counts(members, truth, thresholds)
    M = len(members) if M is None else M
    table, nbh, cells, nan_cells = tables(n, o, nan, M, list(halves))
    return dict(n=n, o=o, nan=nan, table=table, nbh=nbh, cells=cells, nan_cells=nan_cells,
                scores=finish(M, table, nbh, cells))


def finish(M, table, nbh, cells):
    """the header's formulas, in its order; every value a Python float.  Returns a dict of lists per threshold"""
    nt, ns = table.shape[0], nbh.shape[1]
    out = dict(brier=[], reliability=[], resolution=[], uncertainty=[], roc_area=[], fss=[], hit_rate=[], false_alarm=[])
    n = int(cells)
    for q in range(nt):
        T = [[int(table[q, k, 0]), int(table[q, k, 1])] for k in range(M + 1)]
        SO = sum(t[1] for t in T)
        hit, fa = [NAN] * (M + 1), [NAN] * (M + 1)
        if n == 0:
            b = rel = res = unc = area = NAN
        else:
            dn = float(n)
            obar = float(SO) / dn
            b = rel = res = 0.0
            for k in range(M + 1):
                p = float(k) / float(M)
                pm = p - 1.0
                t0 = (p * p) * float(T[k][0])
                t1 = (pm * pm) * float(T[k][1])
                b = b + (t0 + t1)
                N = T[k][0] + T[k][1]
                if N > 0:
                    dN = float(N)
                    f = float(T[k][1]) / dN
                    d1, d2 = p - f, f - obar
                    rel = rel + dN * (d1 * d1)
                    res = res + dN * (d2 * d2)
            b, rel, res = b / dn, rel / dn, res / dn
            unc = obar * (1.0 - obar)
            no_event, no_miss = SO == 0, SO == n
            ch = cf = 0
            area, hp, fp = 0.0, 0.0, 0.0
            for k in range(M, -1, -1):
                ch += T[k][1]
                cf += T[k][0]
                hk = NAN if no_event else float(ch) / float(SO)
                fk = NAN if no_miss else float(cf) / float(n - SO)
                hit[k], fa[k] = hk, fk
                if not no_event and not no_miss:
                    area = area + ((fk - fp) * (hk + hp)) * 0.5
                hp, fp = hk, fk
            if no_event or no_miss:
                area = NAN
        fss = []
        for s in range(ns):
            A, Bo, Cc = (int(v) for v in nbh[q, s])
            S = A + M * M * Bo
            D = S - 2 * M * Cc
            assert 0 <= D <= S < 2 ** 64
            fss.append(NAN if S == 0 else 1.0 - float(D) / float(S))
        for k, v in zip(("brier", "reliability", "resolution", "uncertainty", "roc_area", "fss", "hit_rate",
                         "false_alarm"), (b, rel, res, unc, area, fss, hit, fa)):
            out[k].append(v)
    return out


def same_bits(a, b):
    """equal as IEEE doubles bit for bit, any NaN matching any NaN (a NaN's sign and payload are not specified)"""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def scores_match(got, want):
    """got: SpatialScores of the package; want: finish()'s dict.  The names that differ"""
    bad = [k for k in ("brier", "reliability", "resolution", "uncertainty", "roc_area", "fss", "hit_rate", "false_alarm")
           if not same_bits(getattr(got, k), np.asarray(want[k], dtype=np.float64))]
    return bad


def fsum_brier_terms(table_q, M):
    """math.fsum of (k / M - b)^2 repeated table_q[k][b] times: the exactly rounded sum of the grid-scale Brier terms"""
    terms = []
    for k in range(M + 1):
        for b in (0, 1):
            d = float(k) / float(M) - float(b)
            terms += [d * d] * int(table_q[k][b])
    return math.fsum(terms)
