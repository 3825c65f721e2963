"""Per-cell ensemble quantiles and exceedance probabilities (csim_ensemble_quantiles*): against np.quantile(a, q, axis=0)
and np.mean(a > t, axis=0) of download_all(), whole arrays, ghost ring included.  Quantiles must equal numpy by
integer view wherever numpy's value is non-zero and not NaN (the sign of a zero is left open, as numpy's partition
leaves it), and np.array_equal(equal_nan=True) everywhere; exceedance bit for bit."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from test_gpu_ensemble import PHYS12, random_fields

pytestmark = pytest.mark.gpu

LEVELS = [0.0, 0.1, 1 / 3, 0.5, 0.9, 0.999999, 1.0]


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


def assert_quantiles(got, a, qs, ts, what):
    assert got.q.shape == (len(qs),) + a.shape[1:], what
    assert got.exceed.shape == (len(ts),) + a.shape[1:], what
    with np.errstate(all="ignore"):
        for k, q in enumerate(qs):
            want = np.quantile(a, q, axis=0)
            assert np.array_equal(got.q[k], want, equal_nan=True), f"{what}: q = {q}"
            exact = (want != 0) & ~np.isnan(want)
            assert np.array_equal(got.q[k][exact].view(np.int64), want[exact].view(np.int64)), f"{what}: q = {q} bits"
        for k, t in enumerate(ts):
            want = np.mean(a > t, axis=0)
            assert np.array_equal(got.exceed[k].view(np.int64), want.view(np.int64)), f"{what}: t = {t}"


def check(csim, e, qs=LEVELS, ts=(0.0, 0.5), what=""):
    a = e.download_all()
    assert_quantiles(e.quantiles(qs, ts), a, list(qs), list(ts), what)
    return a


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 32, 33, 63, 64, 65, 100, 128, 129, 255, 256, 257, 1000])
@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (130, 67)])
def test_members_and_shapes(csim, B, shape):
    nx, ny = shape
    e = ensemble_with(csim, random_fields(B, nx, ny, seed=B * 7 + nx))
    check(csim, e, what=f"{B} x {nx}x{ny}")


@pytest.mark.parametrize("B", [4, 64, 100])
def test_512x512(csim, B):
    e = ensemble_with(csim, random_fields(B, 512, 512, seed=B))
    check(csim, e, qs=[0.1, 0.5, 0.9], ts=[0.0, 1.0], what=f"{B} x 512^2")


@pytest.mark.parametrize("B", [2047, 2048, 2049, 4095, 4096])
def test_largest_networks(csim, B):
    u0s = nasty_members(B, 1, 1, seed=B)
    e = ensemble_with(csim, u0s)
    check(csim, e, ts=(-np.inf, 0.0, 1e308), what=f"{B} x 1x1")


@pytest.mark.parametrize("bcs", ["dddd", "nnnn", "dnpd"])
@pytest.mark.parametrize("steps", [0, 1, 4, 7, 23])
def test_after_runs_130x67(csim, bcs, steps):
    u0s = random_fields(12, 130, 67, seed=300 + steps)
    e = ensemble_with(csim, u0s, csim.bc_codes(bcs))
    if steps:
        e.set_physics(*[[p[k] for p in PHYS12] for k in range(4)])
        e.run(steps)
    check(csim, e, what=f"{bcs} {steps} steps")


def nasty_members(B, nx, ny, seed):
    """special values scattered, plus cells built to hit numpy's quirks (ghost ring included)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((B, ny + 2, nx + 2))
    pick = lambda n: tuple(rng.integers(0, [B, ny + 2, nx + 2], size=(n, 3)).T)  # noqa: E731
    cells = (ny + 2) * (nx + 2)
    for v, n in [(np.inf, 3), (-np.inf, 3), (0.0, 4), (-0.0, 4), (5e-324, 2), (-5e-324, 2), (2.2e-308, 2)]:
        a[pick(max(1, n * cells * B // 100))] = v
    if cells >= 12:
        a[:, 0, 0] = np.inf                       # every chosen statistic +inf: inf - inf gives NaN
        a[:, 0, 1] = -np.inf
        a[:, 0, 2] = 0.25                         # all members equal
        a[:, 1, 0] = rng.choice([-0.0, 0.0], B)   # signed zeros only
        a[:, 1, 1] = rng.choice([-1.0, 0.0, 1.0, 2.0], B)  # many ties
        a[:, 1, 2] = rng.choice([5e-324, -5e-324, 1e-310, -2.2e-308], B)  # subnormals
        a[:, 2, 0] = np.nan                       # every member NaN
        a[B // 2, 2, 1] = np.nan                  # one NaN member
        a[:, 2, 2] = np.where(np.arange(B) < B // 2, -np.inf, np.inf)  # half -inf, half +inf
        a[: B // 3, 3, 0] = np.inf                # the top third +inf
    else:
        a[B // 2, 0, 0] = np.nan
        a[: B // 3, 0, 1] = np.inf
        a[: B // 3, 0, 2] = -np.inf
    return a


@pytest.mark.parametrize("B", [1, 2, 3, 5, 12, 31, 64, 65, 100, 256, 257, 600])
def test_special_values(csim, B):
    e = ensemble_with(csim, nasty_members(B, 9, 5, seed=B))
    a = e.download_all()
    vals = sorted(set(a[:, 1, 1].tolist()))
    ts = [-np.inf, np.inf, np.nan, 0.0, -0.0, vals[0], vals[-1], 0.25, 5e-324]
    got = e.quantiles(LEVELS, ts)
    assert_quantiles(got, a, LEVELS, ts, f"special values, B = {B}")
    assert np.isnan(got.q[:, 2, 0]).all() and (got.exceed[:, 2, 0] == 0).all()
    assert (got.exceed[2] == 0).all()  # NaN threshold


def test_nan_in_one_member(csim):
    B = 12
    u0s = random_fields(B, 16, 8, seed=11)
    u0s[5, 3, 4] = np.nan
    e = ensemble_with(csim, u0s)
    got = e.quantiles([0.0, 0.5, 1.0], [0.0])
    assert np.isnan(got.q[:, 3, 4]).all()
    assert np.isnan(got.q).sum() == 3
    assert_quantiles(got, e.download_all(), [0.0, 0.5, 1.0], [0.0], "one NaN")


def test_levels_with_exact_indices(csim):
    for B in (5, 12, 64, 65, 257):
        e = ensemble_with(csim, random_fields(B, 20, 10, seed=B))
        qs = [k / (B - 1) for k in (1, 2, B // 2, B - 2)] + [1e-300, 0.999999]
        check(csim, e, qs=qs[:16], ts=(), what=f"exact indices, B = {B}")


def test_sixteen_levels_and_thresholds(csim):
    e = ensemble_with(csim, random_fields(40, 33, 17, seed=40))
    qs = list(np.linspace(0, 1, 16))
    ts = list(np.linspace(-2, 2, 16))
    check(csim, e, qs=qs, ts=ts, what="16 + 16")
    check(csim, e, qs=[], ts=ts[:3], what="thresholds only")
    check(csim, e, qs=qs[:2], ts=[], what="levels only")


def test_null_outputs_are_skipped(csim):
    e = ensemble_with(csim, random_fields(7, 20, 10, seed=3))
    a = e.download_all()
    lib, C = csim.lib(), csim.C
    q = np.array([0.5, 0.25])
    t = np.array([0.0])
    p = np.full((1, 12, 22), 7.0)
    dp = C.POINTER(C.c_double)
    assert lib.csim_ensemble_quantiles(e._h, 2, q.ctypes.data_as(dp), 1, t.ctypes.data_as(dp), None,
                                       p.ctypes.data_as(dp)) == 0
    assert np.array_equal(p[0], np.mean(a > 0.0, axis=0))
    assert lib.csim_ensemble_quantiles(e._h, 2, q.ctypes.data_as(dp), 1, t.ctypes.data_as(dp), None, None) == 0


def test_async_captures_the_state_before_the_run(csim):
    bc = csim.bc_codes("dnpd")
    u0s = random_fields(70, 130, 67, seed=42)
    phys = [[PHYS12[m % 12][k] for m in range(70)] for k in range(4)]
    e, plain = ensemble_with(csim, u0s, bc), ensemble_with(csim, u0s, bc)
    e.set_physics(*phys)
    plain.set_physics(*phys)
    qs, ts = [0.1, 0.5, 0.9], [0.0]
    for k in (7, 20, 1):
        before = e.download_all()
        sync = e.quantiles(qs, ts)
        e.quantiles_begin(qs, ts)
        e.run(k)
        got = e.quantiles_wait()
        assert np.array_equal(got.q, sync.q, equal_nan=True) and np.array_equal(got.exceed, sync.exceed)
        assert_quantiles(got, before, qs, ts, f"begin; run({k}); wait")
        plain.run(k)
        assert np.array_equal(e.download_all(), plain.download_all()), f"run({k}) changed by the quantiles"
    # two _begin in a row: the second one's state, with its own levels
    e.quantiles_begin(qs, ts)
    e.run(4)
    e.quantiles_begin([0.5], [0.0, 1.0, 2.0])
    now = e.download_all()
    assert_quantiles(e.quantiles_wait(), now, [0.5], [0.0, 1.0, 2.0], "second begin")
    # a synchronous call between _begin and _wait leaves the captured result alone
    e.quantiles_begin(qs, ts)
    e.run(3)
    e.quantiles(list(np.linspace(0, 1, 16)), list(np.linspace(-1, 1, 16)))
    assert_quantiles(e.quantiles_wait(), now, qs, ts, "begin; run; quantiles; wait")
    with pytest.raises(csim.CsimError) as ex:
        e.quantiles_wait()  # nothing in flight any more
    assert ex.value.code == 4


@pytest.mark.parametrize("stats_first", [True, False])
def test_stats_and_quantiles_in_flight_together(csim, stats_first):
    u0s = random_fields(100, 64, 48, seed=7)
    e = ensemble_with(csim, u0s)
    e.set_physics(*[[PHYS12[m % 12][k] for m in range(100)] for k in range(4)])
    e.run(5)
    before = e.download_all()
    qs, ts = [0.05, 0.5, 0.95], [0.0, -1.0]
    if stats_first:
        e.stats_begin(1)
        e.quantiles_begin(qs, ts)
    else:
        e.quantiles_begin(qs, ts)
        e.stats_begin(1)
    e.run(9)
    if stats_first:
        st = e.stats_wait()
        got = e.quantiles_wait()
    else:
        got = e.quantiles_wait()
        st = e.stats_wait()
    assert_quantiles(got, before, qs, ts, "with stats in flight")
    assert np.array_equal(st.mean, np.mean(before, axis=0))
    assert np.array_equal(st.max, before.max(axis=0))


def test_fields_untouched(csim):
    bc = csim.bc_codes("nnnn")
    u0s = random_fields(12, 40, 30, seed=9)
    phys = [[p[k] for p in PHYS12] for k in range(4)]
    e, plain = ensemble_with(csim, u0s, bc), ensemble_with(csim, u0s, bc)
    for x in (e, plain):
        x.set_physics(*phys)
        x.run(6)
    e.quantiles([0.5], [0.0])
    e.run(11)
    plain.run(11)
    assert np.array_equal(e.download_all().view(np.int64), plain.download_all().view(np.int64))


def test_errors(csim):
    E = csim.CsimError
    e = csim.Ensemble(3, 8, 8)
    with pytest.raises(E) as ex:
        e.quantiles_wait()  # never begun
    assert ex.value.code == 4
    bad_calls = [
        lambda: e.quantiles([], []),                  # nq + nt = 0
        lambda: e.quantiles([-0.1]),
        lambda: e.quantiles([1.5]),
        lambda: e.quantiles([np.nan]),
        lambda: e.quantiles([0.5] * 17),
        lambda: e.quantiles([0.5], [0.0] * 17),
        lambda: e.quantiles_begin([0.5, 2.0]),
        lambda: e.quantiles_begin([], []),
    ]
    for bad in bad_calls:
        with pytest.raises(E) as ex:
            bad()
        assert ex.value.code == 1
    lib, C = csim.lib(), csim.C
    d1 = (C.c_double * 1)(0.5)
    assert lib.csim_ensemble_quantiles(e._h, -1, d1, 1, d1, None, None) == 1
    assert lib.csim_ensemble_quantiles(e._h, 1, d1, -1, d1, None, None) == 1
    assert lib.csim_ensemble_quantiles(e._h, 1, None, 0, None, None, None) == 1
    with pytest.raises(E) as ex:
        e.quantiles_wait()  # the refused _begin left nothing in flight
    assert ex.value.code == 4
    check(csim, e, what="after errors")


def test_member_limit(csim):
    big = csim.Ensemble(4097, 1, 1)
    with pytest.raises(csim.CsimError) as ex:
        big.quantiles([0.5])
    assert ex.value.code == 5
    assert "4096" in str(ex.value)
    with pytest.raises(csim.CsimError) as ex:
        big.quantiles_begin([0.5])
    assert ex.value.code == 5
    big.close()
