"""Ensemble verification (csim_ensemble_verify*): per-cell CRPS and Brier scores, rank histogram and domain scores
against a numpy restatement of the definition in include/csim.h, bit for bit, plus an independent check of the CRPS
against its pairwise definition."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from test_gpu_ensemble import PHYS12, random_fields

pytestmark = pytest.mark.gpu

THR = [0.0, 0.5]


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def ensemble_with(csim, u0s, bc=(0, 0, 0, 0)):
    B, ny2, nx2 = u0s.shape
    e = csim.Ensemble(B, nx2 - 2, ny2 - 2, 1.0, 1.0, bc)
    e.upload_all(u0s)
    return e


# ---- the restatement ---------------------------------------------------------------------------------------------

def ordered_sum(terms, first=0):
    """sum over axis 0 of terms[k] for k = first .. len - 1 (index k), in the kernel's order: one running sum from +0
    for M <= 64; above that lane k % 64 sums its terms in increasing k and the 64 lane sums go through an xor tree"""
    M = terms.shape[0]
    if M <= 64:
        acc = np.zeros(terms.shape[1:])
        for k in range(first, M):
            acc = acc + terms[k]
        return acc
    lanes = np.zeros((64,) + terms.shape[1:])
    for k in range(first, M):
        lanes[k % 64] = lanes[k % 64] + terms[k]
    for h in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ h]
    return lanes[0]


def mix(g):
    z = np.asarray(g, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def restate(x, y, thr, fair):
    """x: (M, ny+2, nx+2) forecast, y: (ny+2, nx+2) truth -> crps, brier, hist, per-cell (nan, mean, var)"""
    M = x.shape[0]
    with np.errstate(all="ignore"):
        nan = np.isnan(y) | np.isnan(x).any(axis=0)
        a = ordered_sum(np.abs(x - y))
        m = ordered_sum(x) / float(M)
        v = ordered_sum((x - m) * (x - m)) / float(M - 1)
        s = np.sort(x, axis=0)
        w = np.array([float(i * (M - i)) for i in range(M)]).reshape((M,) + (1,) * (x.ndim - 1))
        gaps = np.concatenate([np.zeros((1,) + x.shape[1:]), w[1:] * (s[1:] - s[:-1])])
        c = ordered_sum(gaps, first=1)
        W = float(M * (M - 1) if fair else M * M)
        crps = np.where(nan, np.nan, a / float(M) - c / W)
        brier = []
        for t in thr:
            p = (x > t).sum(axis=0) / float(M)
            o = np.where(y > t, 1.0, 0.0)
            brier.append(np.where(nan, np.nan, (p - o) * (p - o)))
        brier = np.array(brier).reshape((len(thr),) + y.shape)
        ny, nx = y.shape[0] - 2, y.shape[1] - 2
        inner = np.zeros(y.shape, dtype=bool)
        inner[1:-1, 1:-1] = True
        lt = (x < y).sum(axis=0)
        eq = (x == y).sum(axis=0)
        jj, ii = np.meshgrid(np.arange(ny + 2), np.arange(nx + 2), indexing="ij")
        g = ((jj - 1) * nx + (ii - 1)).clip(0).astype(np.uint64)
        rank = lt + (mix(g) % (eq + 1).astype(np.uint64)).astype(np.int64)
        ok = inner & ~nan
        hist = np.bincount(rank[ok], minlength=M + 1).astype(np.uint64)
    return crps, brier, hist, dict(nan=nan, ok=ok, inner=inner, m=m, v=v)


def same(got, want):
    """bit for bit where want is a number, NaN where want is NaN"""
    n = np.isnan(want)
    return np.array_equal(np.isnan(got), n) and np.array_equal(got[~n].view(np.int64), want[~n].view(np.int64))


def same_scores(a, b):
    return a[:2] == b[:2] and same(np.array(a[2:5]), np.array(b[2:5])) and same(a.brier, b.brier)


def close(got, want, rel=1e-12, tiny=1e-300):
    if np.isnan(want):
        return np.isnan(got)
    if got == want:
        return True
    return abs(got - want) <= rel * abs(want) + tiny


def check_all(got, x, y, thr, fair, what):
    crps, brier, hist, d = restate(x, y, thr, fair)
    assert same(got.crps, crps), f"{what}: crps"
    assert got.brier.shape == brier.shape and same(got.brier, brier), f"{what}: brier"
    assert got.rank_hist.dtype == np.uint64 and np.array_equal(got.rank_hist, hist), f"{what}: rank histogram"
    sc, ok = got.scores, d["ok"]
    assert sc.cells == int(ok.sum()) and sc.nan_cells == int((d["inner"] & d["nan"]).sum()), what
    if ok.any():
        with np.errstate(all="ignore"):
            assert close(sc.crps, np.mean(crps[ok])), f"{what}: mean crps"
            assert close(sc.rmse, np.sqrt(np.mean((d["m"] - y)[ok] ** 2))), f"{what}: rmse"
            assert close(sc.spread, np.sqrt(np.mean(d["v"][ok]))), f"{what}: spread"
            for k in range(len(thr)):
                assert close(sc.brier[k], np.mean(brier[k][ok])), f"{what}: brier {k}"
    else:
        assert np.isnan(sc.crps) and np.isnan(sc.rmse) and np.isnan(sc.spread)
    return crps, d


def pairwise_crps(x, y, fair):
    M = x.shape[0]
    mae = np.mean(np.abs(x - y), axis=0)
    pair = np.zeros(y.shape)
    for i in range(M):
        pair += np.abs(x - x[i]).sum(axis=0)
    return mae - pair / (2.0 * (M * (M - 1) if fair else M * M))


# ---- tests -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 100, 128, 129, 256, 257, 1000])
@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (130, 67)])
def test_members_and_shapes(csim, M, shape):
    nx, ny = shape
    x = random_fields(M, nx, ny, seed=M * 7 + nx)
    y = np.random.default_rng(M).random((ny + 2, nx + 2))
    e = ensemble_with(csim, x)
    for fair in ([False, True] if M >= 2 else [False]):
        got = e.verify(y, thresholds=THR, fair=fair)
        crps, _ = check_all(got, x, y, THR, fair, f"M = {M}, {nx}x{ny}, fair = {fair}")
        rows = slice(0, 3)  # the pairwise sum costs M^2 per cell
        want = pairwise_crps(x[:, rows], y[rows], fair)
        assert np.allclose(crps[rows], want, rtol=1e-12, atol=1e-13), f"M = {M}: pairwise definition"
    if M == 1:
        assert np.array_equal(got.crps, np.abs(x[0] - y))


@pytest.mark.parametrize("M", [4, 64, 100])
def test_512x512(csim, M):
    x = random_fields(M, 512, 512, seed=M)
    y = random_fields(1, 512, 512, seed=M + 1)[0]
    e = ensemble_with(csim, x)
    check_all(e.verify(y, thresholds=[0.25, 0.75, 0.5]), x, y, [0.25, 0.75, 0.5], False, f"{M} x 512^2")


@pytest.mark.parametrize("M", [2048, 2049, 4095, 4096])
def test_largest_networks(csim, M):
    x = np.random.default_rng(M).standard_normal((M, 3, 3))
    x[: M // 3, 0, 1] = 0.5  # ties with the truth
    y = np.random.default_rng(M + 1).standard_normal((3, 3))
    y[0, 1] = 0.5
    e = ensemble_with(csim, x)
    for fair in (False, True):
        check_all(e.verify(y, thresholds=[0.0, 0.5], fair=fair), x, y, [0.0, 0.5], fair, f"{M} x 1x1")


def test_truth_member_4097(csim):
    a = np.random.default_rng(4097).standard_normal((4097, 3, 3))
    e = ensemble_with(csim, a)
    got = e.verify(truth_member=17, thresholds=[0.1])
    check_all(got, np.delete(a, 17, axis=0), a[17], [0.1], False, "B = 4097, truth member")
    with pytest.raises(csim.CsimError) as ex:
        e.verify(a[0])  # M = 4097
    assert ex.value.code == 5


@pytest.mark.parametrize("B,t", [(2, 0), (3, 2), (13, 5), (65, 0), (66, 64), (101, 50), (300, 299)])
def test_truth_sources_agree(csim, B, t):
    a = random_fields(B, 33, 17, seed=B + t)
    e = ensemble_with(csim, a)
    rest = ensemble_with(csim, np.delete(a, t, axis=0))
    for fair in ([False, True] if B >= 3 else [False]):
        got = e.verify(truth_member=t, thresholds=THR, fair=fair)
        ref = rest.verify(e.download(t), thresholds=THR, fair=fair)
        for f in ("crps", "brier", "rank_hist"):
            assert np.array_equal(getattr(got, f).view(np.int64), getattr(ref, f).view(np.int64)), f
        assert same_scores(got.scores, ref.scores)
        check_all(got, np.delete(a, t, axis=0), a[t], THR, fair, f"B = {B}, t = {t}")


@pytest.mark.parametrize("bcs", ["dddd", "nnnn", "dnpd"])
def test_twin_experiment(csim, bcs):
    bc = csim.bc_codes(bcs)
    B, nx, ny, steps = 24, 96, 72, 40
    D, vx, vy = 0.05, 0.5, -0.25
    rng = np.random.default_rng(8)
    Ds = D * (1 + 0.3 * rng.uniform(-1, 1, B))
    vxs = vx + 0.2 * rng.uniform(-1, 1, B)
    vys = vy + 0.2 * rng.uniform(-1, 1, B)
    Ds[0], vxs[0], vys[0] = D, vx, vy  # member 0: the control run
    dt = min([0.1] + [csim.safe_dt(1.0, 1.0, vxs[m], vys[m], Ds[m]) for m in range(B)])
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, bc)
    for m in range(B):
        e.init_gaussian(m, 1.0, 0.08, 0.4, 0.5)
    e.set_physics(Ds, dt, vxs, vys)
    e.run(steps)
    a = e.download_all()
    got = e.verify(truth_member=0, thresholds=[0.01, 0.1])
    check_all(got, a[1:], a[0], [0.01, 0.1], False, f"twin {bcs}")
    single = csim.Ensemble(1, nx, ny, 1.0, 1.0, bc)
    single.init_gaussian(0, 1.0, 0.08, 0.4, 0.5)
    single.set_physics(D, dt, vx, vy)
    single.run(steps)
    assert np.array_equal(single.download(0).view(np.int64), a[0].view(np.int64))
    assert got.scores.cells == nx * ny and got.scores.nan_cells == 0


@pytest.mark.parametrize("M", [1, 5, 64, 65, 200])
def test_ties_and_special_values(csim, M):
    rng = np.random.default_rng(M)
    nx, ny = 9, 6
    x = rng.standard_normal((M, ny + 2, nx + 2))
    y = rng.standard_normal((ny + 2, nx + 2))
    x[:, 2, 2] = y[2, 2]                                   # all members equal to the truth
    x[:, 2, 3] = rng.choice([-0.0, 0.0], M)                # a +-0 mix against +0
    y[2, 3] = 0.0
    x[:, 2, 4] = rng.choice([-0.0, 0.0], M)                # ... and against -0
    y[2, 4] = -0.0
    x[: (M + 1) // 2, 3, 3] = np.inf                       # +inf members
    x[M // 2:, 3, 4] = -np.inf                             # -inf members
    y[3, 5] = np.inf                                       # an infinite truth
    x[M // 2, 4, 4] = np.nan                               # one NaN member
    y[4, 5] = np.nan                                       # a NaN truth cell
    x[:, 5, 1] = rng.choice([-1.0, 0.0, 1.0], M)           # many ties
    y[5, 1] = 0.0
    e = ensemble_with(csim, x)
    got = e.verify(y, thresholds=[0.0, -0.0, np.inf, -np.inf])
    crps, d = check_all(got, x, y, [0.0, -0.0, np.inf, -np.inf], False, f"special values, M = {M}")
    assert got.scores.nan_cells == 2 and np.isnan(got.crps[4, 4]) and np.isnan(got.crps[4, 5])
    assert np.isnan(got.brier[:, 4, 4]).all()
    assert got.crps[2, 2] == 0.0
    assert got.scores.cells == nx * ny - 2 and int(got.rank_hist.sum()) == nx * ny - 2


def test_dirichlet_ring_ties_spread(csim):
    """members that equal the truth everywhere: every cell is a tie of all M members, so its bin is mix(g) mod (M+1)"""
    M, nx, ny = 7, 40, 30
    x = np.zeros((M, ny + 2, nx + 2))
    e = ensemble_with(csim, x)
    got = e.verify(np.zeros((ny + 2, nx + 2)))
    g = np.arange(nx * ny, dtype=np.uint64)
    with np.errstate(over="ignore"):
        want = np.bincount((mix(g) % np.uint64(M + 1)).astype(np.int64), minlength=M + 1)
    assert np.array_equal(got.rank_hist, want.astype(np.uint64))
    assert (got.rank_hist > 0).all() and got.rank_hist.max() < nx * ny // 4  # no pile-up in bin 0
    assert (got.crps == 0).all() and got.scores.crps == 0.0 and got.scores.rmse == 0.0


def test_scores_repeatable_and_rmse_is_stats_mean(csim):
    x = random_fields(80, 200, 150, seed=3)
    y = random_fields(1, 200, 150, seed=4)[0]
    e = ensemble_with(csim, x)
    r1, r2 = e.verify(y, thresholds=THR), e.verify(y, thresholds=THR)
    assert same_scores(r1.scores, r2.scores)
    st = e.stats(1)
    sq = ((st.mean - y)[1:-1, 1:-1]) ** 2
    assert close(r1.scores.rmse, np.sqrt(np.mean(sq)))
    assert close(r1.scores.spread, np.sqrt(np.mean(st.var[1:-1, 1:-1])))


def test_async_captures_the_state_before_the_run(csim):
    bc = csim.bc_codes("dnpd")
    B = 70
    u0s = random_fields(B, 130, 67, seed=42)
    phys = [[PHYS12[m % 12][k] for m in range(B)] for k in range(4)]
    e, plain = ensemble_with(csim, u0s, bc), ensemble_with(csim, u0s, bc)
    e.set_physics(*phys)
    plain.set_physics(*phys)
    y = random_fields(1, 130, 67, seed=43)[0]
    for k, tm in ((7, None), (20, 3), (1, None)):
        before = e.download_all()
        kw = dict(truth_member=tm) if tm is not None else dict(truth=y.copy())
        sync = e.verify(**kw, thresholds=THR)
        truth = kw.get("truth")
        e.verify_begin(**kw, thresholds=THR)
        if truth is not None:
            truth[:] = -5.0  # the call copied it
        e.run(k)
        got = e.verify_wait()
        for f in ("crps", "brier", "rank_hist"):
            assert np.array_equal(getattr(got, f).view(np.int64), getattr(sync, f).view(np.int64)), f
        assert same_scores(got.scores, sync.scores)
        x, yy = (np.delete(before, tm, axis=0), before[tm]) if tm is not None else (before, y)
        check_all(got, x, yy, THR, False, f"begin; run({k}); wait")
        plain.run(k)
        assert np.array_equal(e.download_all(), plain.download_all()), f"run({k}) changed by the verification"
    # a synchronous call between _begin and _wait leaves the captured result alone
    now = e.download_all()
    e.verify_begin(y, thresholds=THR)
    e.run(3)
    e.verify(truth_member=0, thresholds=[0.1, 0.2, 0.3], fair=True)
    check_all(e.verify_wait(), now, y, THR, False, "begin; run; verify; wait")
    with pytest.raises(csim.CsimError) as ex:
        e.verify_wait()
    assert ex.value.code == 4


@pytest.mark.parametrize("verify_first", [True, False])
def test_in_flight_with_stats_and_quantiles(csim, verify_first):
    u0s = random_fields(100, 64, 48, seed=7)
    e = ensemble_with(csim, u0s)
    e.set_physics(*[[PHYS12[m % 12][k] for m in range(100)] for k in range(4)])
    e.run(5)
    before = e.download_all()
    if verify_first:
        e.verify_begin(truth_member=1, thresholds=THR)
        e.stats_begin(1)
        e.quantiles_begin([0.5], [0.0])
    else:
        e.quantiles_begin([0.5], [0.0])
        e.stats_begin(1)
        e.verify_begin(truth_member=1, thresholds=THR)
    e.run(9)
    got = e.verify_wait()
    st = e.stats_wait()
    q = e.quantiles_wait()
    check_all(got, np.delete(before, 1, axis=0), before[1], THR, False, "with stats and quantiles in flight")
    assert np.array_equal(st.mean, np.mean(before, axis=0))
    assert np.array_equal(q.exceed[0], np.mean(before > 0.0, axis=0))


def test_null_outputs_and_fields_untouched(csim):
    bc = csim.bc_codes("nnnn")
    u0s = random_fields(12, 40, 30, seed=9)
    phys = [[p[k] for p in PHYS12] for k in range(4)]
    e, plain = ensemble_with(csim, u0s, bc), ensemble_with(csim, u0s, bc)
    for z in (e, plain):
        z.set_physics(*phys)
        z.run(6)
    a = e.download_all()
    lib, C = csim.lib(), csim.C
    dp = C.POINTER(C.c_double)
    t = np.array([0.0])
    crps = np.full((32, 42), 7.0)
    assert lib.csim_ensemble_verify(e._h, None, 0, 0, 1, t.ctypes.data_as(dp), crps.ctypes.data_as(dp), None, None,
                                    None) == 0
    want, _, _, _ = restate(a[1:], a[0], [0.0], False)
    assert same(crps, want)
    assert lib.csim_ensemble_verify(e._h, None, 0, 0, 1, t.ctypes.data_as(dp), None, None, None, None) == 0
    assert lib.csim_ensemble_verify_begin(e._h, None, 2, 1, 0, None) == 0
    assert lib.csim_ensemble_verify_wait(e._h, None, None, None, None) == 0
    e.run(11)
    plain.run(11)
    assert np.array_equal(e.download_all().view(np.int64), plain.download_all().view(np.int64))


def test_errors(csim):
    E = csim.CsimError
    e = csim.Ensemble(3, 8, 8)
    y = np.zeros((10, 10))
    with pytest.raises(E) as ex:
        e.verify_wait()
    assert ex.value.code == 4
    lib, C = csim.lib(), csim.C
    dp = C.POINTER(C.c_double)
    yp = y.ctypes.data_as(dp)
    t1 = (C.c_double * 17)(*([0.0] * 17))
    bad = [
        (None, -1, 0, 0, None),   # no truth
        (yp, 0, 0, 0, None),      # both truths
        (None, 3, 0, 0, None),    # truth member out of range
        (None, -2, 0, 0, None),
        (yp, -2, 0, 0, None),
        (yp, -1, 2, 0, None),     # fair not 0 / 1
        (yp, -1, -1, 0, None),
        (yp, -1, 0, -1, t1),      # nt out of range
        (yp, -1, 0, 17, t1),
        (yp, -1, 0, 1, None),     # null thresholds
    ]
    for truth, tm, fair, nt, thr in bad:
        assert lib.csim_ensemble_verify(e._h, truth, tm, fair, nt, thr, None, None, None, None) == 1, (tm, fair, nt)
        assert lib.csim_ensemble_verify_begin(e._h, truth, tm, fair, nt, thr) == 1, (tm, fair, nt)
    with pytest.raises(E) as ex:
        e.verify_wait()  # the refused _begin left nothing in flight
    assert ex.value.code == 4
    one, two = csim.Ensemble(1, 4, 4), csim.Ensemble(2, 4, 4)
    for z, kw in ((one, dict(truth=np.zeros((6, 6)), fair=True)), (one, dict(truth_member=0)),
                  (two, dict(truth_member=1, fair=True))):
        with pytest.raises(E) as ex:
            z.verify(**kw)  # fair with M < 2, or no forecast member
        assert ex.value.code == 1
    big = csim.Ensemble(4098, 1, 1)
    for kw in (dict(truth_member=0), dict(truth=np.zeros((3, 3)))):
        with pytest.raises(E) as ex:
            big.verify(**kw)
        assert ex.value.code == 5
        with pytest.raises(E) as ex:
            big.verify_begin(**kw)
        assert ex.value.code == 5
    x = random_fields(3, 8, 8, seed=1)
    e.upload_all(x)
    check_all(e.verify(y, thresholds=THR), x, y, THR, False, "after errors")
