"""Ensemble analysis (csim_ensemble_assimilate): the serial EnSRF against a numpy restatement of the block in
include/csim.h, bit for bit (fields and diagnostics); what it must leave alone; stepping afterwards against a
single-rank Stepper; pipelining without diagnostics; the textbook Kalman update for one observation; and an OSSE in
which the analysis must pull the ensemble mean towards the truth."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from test_gpu_ensemble import PHYS12

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def same_bits(got, want):
    """the same bits, where a NaN matches any NaN (a NaN made on the host and one made on the GPU may differ in sign)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.int64), want[ok].view(np.int64))


# ---- the restatement ---------------------------------------------------------------------------------------------

def restate(csim, X, dx, dy, i, j, y, r, loc, lam, t, ordered):
    """X: (B, ny+2, nx+2) -> analysed copy, prior mean / var, post mean / var (input order), level count"""
    X = X.copy()
    B, ny2, nx2 = X.shape
    nx, ny = nx2 - 2, ny2 - 2
    F = [m for m in range(B) if m != t]
    M = len(F)
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    ly, lx = (rho.shape[0] - 1) // 2, (rho.shape[1] - 1) // 2
    lev = csim.ensemble_assim_plan(i, j, lx, ly, ordered)
    n = len(i)
    pm, pv = np.empty(n), np.empty(n)
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
            h = [X[m, jo, io] for m in F]
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
            pm[o], pv[o] = hbar, p
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
        qm, qv = np.empty(n), np.empty(n)
        for o in range(n):
            v = [X[m, int(j[o]), int(i[o])] for m in F]
            s = np.float64(0.0)
            for a in v:
                s = s + a
            mean = s / float(M)
            acc = np.float64(0.0)
            for a in v:
                acc = acc + (a - mean) * (a - mean)
            qm[o], qv[o] = mean, acc / float(M - 1)
    return X, pm, pv, qm, qv, int(lev.max()) + 1 if n else 0


def touched(csim, shape, dx, dy, i, j, loc):
    """cells inside some observation's window with rho > 0 (interior only)"""
    ny2, nx2 = shape
    rho = csim.ensemble_gc_table(dx, dy, loc, nx2 - 2, ny2 - 2)
    ly, lx = (rho.shape[0] - 1) // 2, (rho.shape[1] - 1) // 2
    out = np.zeros(shape, dtype=bool)
    for io, jo in zip(i, j):
        for b in range(-ly, ly + 1):
            for a in range(-lx, lx + 1):
                ci, cj = io + a, jo + b
                if 1 <= ci <= nx2 - 2 and 1 <= cj <= ny2 - 2 and rho[b + ly, a + lx] > 0:
                    out[cj, ci] = True
    return out


def make_obs(rng, nx, ny, n, edges=True):
    i = rng.integers(1, nx + 1, n)
    j = rng.integers(1, ny + 1, n)
    if edges and n >= 8:
        # corners, edges and a duplicated cell
        i[:6] = [1, nx, 1, nx, 1, (nx + 1) // 2]
        j[:6] = [1, ny, ny, 1, (ny + 1) // 2, 1]
        i[6], j[6] = i[0], j[0]
        i[7], j[7] = i[4], j[4]
    y = rng.standard_normal(n)
    r = rng.uniform(0.05, 2.0, n)
    return i.astype(np.int32), j.astype(np.int32), y, r


# B, truth member, nx, ny, dx, dy, nobs, loc, inflation, ordered, nasty values
CASES = [
    (2, None, 5, 1, 1.0, 2.0, 6, 50.0, 1.0, False, False),        # M = 2, windows larger than the grid
    (4, 1, 5, 1, 0.5, 1.0, 9, 1.3, 1.1, True, False),             # M = 3
    (17, None, 37, 29, 0.7, 1.3, 40, 2.0, 1.0, False, True),      # M = 17, NaN / +-0 / 1e300 in the members
    (18, 5, 37, 29, 1.0, 0.6, 40, 2.5, 1.1, True, False),         # M = 17 with a truth member
    (41, None, 37, 29, 1.0, 1.0, 40, 3.0, 1.1, True, True),       # M = 41 (the 48-value register form)
    (64, None, 256, 256, 1.0, 1.5, 300, 4.0, 1.0, False, False),  # M = 64
    (65, 0, 37, 29, 1.3, 1.0, 60, 3.0, 1.1, False, True),         # M = 64 with a truth member
    (65, None, 37, 29, 1.0, 1.0, 60, 30.0, 1.0, True, False),     # M = 65, windows larger than the grid
    (256, None, 37, 29, 0.9, 1.1, 25, 2.0, 1.1, False, True),     # M = 256
    (1025, 7, 5, 1, 1.0, 1.0, 8, 1.0, 1.0, False, False),         # M = 1024, the largest
]


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}_t{c[1]}_{c[2]}x{c[3]}_ord{int(c[9])}" for c in CASES])
def test_restatement_bit_for_bit(csim, case):
    B, t, nx, ny, dx, dy, nobs, loc, lam, ordered, nasty = case
    rng = np.random.default_rng(B * 1000 + nx)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    if nasty:
        X[1, 1, 1] = np.nan
        X[2, ny, nx] = 1e300
        X[:, 2 % ny + 1, 1] = 0.0
        X[0, 2 % ny + 1, 1] = -0.0
        X[3, (ny + 1) // 2, (nx + 1) // 2] = -1e300
    i, j, y, r = make_obs(rng, nx, ny, nobs)
    e = csim.Ensemble(B, nx, ny, dx, dy, (0, 1, 2, 0))
    e.upload_all(X)
    got = e.assimilate(i, j, y, r, loc, inflation=lam, truth_member=t, ordered=ordered)
    G = e.download_all()
    W, pm, pv, qm, qv, nl = restate(csim, X, dx, dy, i, j, y, r, loc, lam, -1 if t is None else t, ordered)
    assert got.nlevels == nl
    for m in range(B):
        assert same_bits(G[m], W[m]), f"member {m} differs from the restatement"
    for name, a, b in (("prior_mean", got.prior_mean, pm), ("prior_var", got.prior_var, pv),
                       ("post_mean", got.post_mean, qm), ("post_var", got.post_var, qv)):
        assert same_bits(a, b), name
    # left alone: the ghost ring, the cells outside every window (with lambda = 1), the truth member
    ring = np.ones((ny + 2, nx + 2), dtype=bool)
    ring[1:-1, 1:-1] = False
    assert same_bits(G[:, ring], X[:, ring])
    if lam == 1.0:
        out = ~touched(csim, (ny + 2, nx + 2), dx, dy, i, j, loc)
        assert same_bits(G[:, out], X[:, out])
    if t is not None:
        assert same_bits(G[t], X[t])
    # a second call on the analysed state: buffers reused, the non-blocking form
    i2, j2, y2, r2 = make_obs(rng, nx, ny, nobs, edges=False)
    W2, *_, nl2 = restate(csim, W, dx, dy, i2, j2, y2, r2, loc, lam, -1 if t is None else t, ordered)
    assert e.assimilate(i2, j2, y2, r2, loc, inflation=lam, truth_member=t, ordered=ordered, diagnostics=False) == nl2
    assert same_bits(e.download_all(), W2)
    e.close()


def test_no_observations(csim):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((6, 12, 9))
    e = csim.Ensemble(6, 7, 10, 1.0, 1.0, (0, 0, 0, 0))
    e.upload_all(X)
    none = np.zeros(0, dtype=np.int32)
    a = e.assimilate(none, none, [], [], 3.0)
    assert a.nlevels == 0 and len(a.prior_mean) == 0
    assert same_bits(e.download_all(), X)
    # inflation alone
    e.assimilate(none, none, [], [], 3.0, inflation=1.25, truth_member=2)
    W = restate(csim, X, 1.0, 1.0, none, none, np.zeros(0), np.zeros(0), 3.0, 1.25, 2, False)[0]
    assert same_bits(e.download_all(), W)
    e.close()


def test_argument_errors(csim):
    e = csim.Ensemble(4, 8, 6, 1.0, 1.0, (0, 0, 0, 0))
    e.upload_all(np.random.default_rng(0).standard_normal((4, 8, 10)))
    ok = dict(i=[1, 8], j=[1, 6], y=[0.0, 1.0], r=[1.0, 1.0], loc=2.0)

    def rejected(code=1, **kw):
        args = dict(ok)
        args.update(kw)
        with pytest.raises(csim.CsimError) as ex:
            e.assimilate(args.pop("i"), args.pop("j"), args.pop("y"), args.pop("r"), args.pop("loc"), **args)
        assert ex.value.code == code, kw

    rejected(i=[0, 8])
    rejected(i=[1, 9])
    rejected(j=[1, 7])
    rejected(j=[0, 6])
    rejected(r=[0.0, 1.0])
    rejected(r=[-1.0, 1.0])
    rejected(r=[np.inf, 1.0])
    rejected(r=[np.nan, 1.0])
    rejected(y=[np.nan, 1.0])
    rejected(y=[np.inf, 1.0])
    rejected(loc=0.0)
    rejected(loc=-1.0)
    rejected(loc=np.inf)
    rejected(loc=np.nan)
    rejected(inflation=0.99)
    rejected(inflation=np.inf)
    rejected(inflation=np.nan)
    rejected(truth_member=4)
    rejected(truth_member=-2)
    lib, C = csim.lib(), csim.C
    ii = (C.c_int * 1)(1)
    dd = (C.c_double * 1)(1.0)
    assert lib.csim_ensemble_assimilate(e._h, 1, ii, ii, dd, dd, 2.0, 1.0, -1, 2, None, None, None, None, None) == 1
    assert lib.csim_ensemble_assimilate(e._h, 1, None, ii, dd, dd, 2.0, 1.0, -1, 0, None, None, None, None, None) == 1
    assert lib.csim_ensemble_assimilate(e._h, 1, ii, ii, dd, None, 2.0, 1.0, -1, 0, None, None, None, None, None) == 1
    assert lib.csim_ensemble_assimilate(e._h, -1, ii, ii, dd, dd, 2.0, 1.0, -1, 0, None, None, None, None, None) == 1
    assert lib.csim_ensemble_assimilate(e._h, 2**20 + 1, ii, ii, dd, dd, 2.0, 1.0, -1, 0, None, None, None, None,
                                        None) == 5
    # nothing was modified by a refused call
    before = e.download_all()
    rejected(i=[1, 9])
    assert same_bits(e.download_all(), before)
    e.close()
    # M < 2: two members with a truth member; M > 1024: unsupported
    e2 = csim.Ensemble(2, 5, 1, 1.0, 1.0, (0, 0, 0, 0))
    with pytest.raises(csim.CsimError) as ex:
        e2.assimilate([1], [1], [0.0], 1.0, 2.0, truth_member=0)
    assert ex.value.code == 1
    e2.close()
    e3 = csim.Ensemble(1025, 5, 1, 1.0, 1.0, (0, 0, 0, 0))
    with pytest.raises(csim.CsimError) as ex:
        e3.assimilate([1], [1], [0.0], 1.0, 2.0)
    assert ex.value.code == 5
    e3.assimilate([1], [1], [0.0], 1.0, 2.0, truth_member=3)  # M = 1024 is allowed
    e3.close()


# ---- stepping afterwards -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("bcs", ["dddd", "nnnn", "dnpd"])
@pytest.mark.parametrize("steps", [3, 9])
def test_stepping_after_analysis_matches_stepper(csim, bcs, steps):
    """assimilate, then run(steps) (9: two fused passes and a single step; 3: single steps only) member by member
    against a single-rank Stepper started from the analysed member"""
    bc = csim.bc_codes(bcs)
    B, nx, ny, dx, dy = 12, 70, 45, 1.0, 0.8
    rng = np.random.default_rng(steps)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    e = csim.Ensemble(B, nx, ny, dx, dy, bc, 0.5)
    e.upload_all(X)
    e.set_physics(*[[p[k] for p in PHYS12] for k in range(4)])
    e.run(5)  # a lived-in state: both buffers, FinLines, ring flags
    i, j, y, r = make_obs(rng, nx, ny, 30)
    e.assimilate(i, j, y, r, 3.0, inflation=1.05, truth_member=4, diagnostics=False)
    start = e.download_all()
    e.run(steps)
    got = e.download_all()
    for m in range(B):
        st = csim.Stepper.single(nx, ny, dx, dy, bc, 0.5)
        st.upload(start[m])
        D, dt, vx, vy = PHYS12[m]
        st.run(D, dt, vx, vy, steps)
        want = st.download()
        st.close()
        assert same_bits(got[m], want), f"member {m}: {bcs}, {steps} steps after the analysis"
    e.close()


def test_pipelining_and_captures(csim):
    B, nx, ny = 20, 96, 64
    rng = np.random.default_rng(11)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, y, r = make_obs(rng, nx, ny, 80)
    runs = []
    for sync in (False, True):
        e = csim.Ensemble(B, nx, ny, 1.0, 1.0, csim.bc_codes("dnpd"))
        e.upload_all(X)
        e.set_physics(0.05, 0.1, 0.5, -0.25)
        e.run(4)
        s0 = e.stats()
        e.stats_begin()
        nl = e.assimilate(i, j, y, r, 4.0, inflation=1.02, diagnostics=sync)
        if sync:
            e.sync()
        e.run(7)
        runs.append(e.download_all())
        cap = e.stats_wait()
        # the capture begun before the analysis sees the state before it
        assert same_bits(cap.mean, s0.mean) and same_bits(cap.var, s0.var)
        e.close()
    assert same_bits(runs[0], runs[1])
    assert nl.nlevels >= 1


# ---- the algorithm, independent of the restatement -----------------------------------------------------------------

def test_single_observation_is_the_kalman_update(csim):
    B, nx, ny = 40, 23, 17
    rng = np.random.default_rng(2)
    base = rng.standard_normal((ny + 2, nx + 2))
    X = base + 0.5 * rng.standard_normal((B, ny + 2, nx + 2))
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    e.upload_all(X)
    io, jo, yo, ro = 9, 7, 1.7, 0.3
    e.assimilate([io], [jo], [yo], ro, 1e12)  # rho = 1 on the whole grid
    A = e.download_all()
    cells = [(jo, io), (1, 1), (ny, nx), (4, 15), (12, 3)]
    Z = np.array([X[:, c[0], c[1]] for c in cells])     # prior samples of the chosen cells
    h = X[:, jo, io]
    P = np.cov(np.vstack([Z, h]))                      # (n+1) x (n+1), the last row is the observed cell
    Pzh, Phh = P[:-1, -1], P[-1, -1]
    K = Pzh / (Phh + ro)
    mean_want = Z.mean(axis=1) + K * (yo - h.mean())
    cov_want = P[:-1, :-1] - np.outer(K, Pzh)
    Za = np.array([A[:, c[0], c[1]] for c in cells])
    np.testing.assert_allclose(Za.mean(axis=1), mean_want, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(np.cov(Za), cov_want, rtol=1e-10, atol=1e-12)
    e.close()


def test_osse_pulls_the_mean_to_the_truth(csim):
    B, nx, ny = 33, 96, 96
    rng = np.random.default_rng(4)
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    e.init_gaussian(0, 1.0, 0.08, 0.5, 0.5)
    for m in range(1, B):
        e.init_gaussian(m, 1.0, 0.08, 0.5 + rng.uniform(-0.12, 0.12), 0.5 + rng.uniform(-0.12, 0.12))
    e.set_physics(0.05, 0.1, 0.3, 0.1)
    e.run(20)
    X = e.download_all()
    truth = X[0, 1:-1, 1:-1]
    g = np.arange(4, nx + 1, 8)
    I, J = np.meshgrid(g, g)
    i, j = I.ravel(), J.ravel()
    sigma = 0.01
    y = X[0, j, i] + sigma * rng.standard_normal(len(i))

    def rmse(F):
        return np.sqrt(np.mean((F[1:, 1:-1, 1:-1].mean(axis=0) - truth) ** 2))

    before = rmse(X)
    a = e.assimilate(i, j, y, sigma * sigma, 6.0, truth_member=0)
    A = e.download_all()
    after = rmse(A)
    assert after < 0.7 * before, (before, after)
    assert same_bits(A[0], X[0])
    # the observed cells moved towards the observations
    assert np.mean(np.abs(a.post_mean - y)) < np.mean(np.abs(a.prior_mean - y))
    e.close()
