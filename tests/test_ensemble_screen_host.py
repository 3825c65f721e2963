"""Host side of the screening of observation networks (csim_obs_network_set_active,
csim_ensemble_assimilate_screened and their kin in include/csim.h), no GPU needed: the entry points are declared and
exported, csim_obs_screen_decide is the restatement's decision (tests/screen_restatement.py) bit for bit on the edges
the header names, and the restatement's screened csim_obs_cycle gives closed forms on dyadic data across the chunk
boundary."""
import numpy as np
import pytest

import obsnet_restatement as obsnet
import screen_restatement as ref
from __graft_entry__ import load_package

NAMES = {"csim_obs_network_set_active": 2, "csim_ensemble_assimilate_screened": 6, "csim_obs_network_screen_log": 4,
         "csim_obs_network_status": 2, "csim_obs_screen_decide": 7}


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    return pkg


def test_entry_points_are_declared_and_exported(csim):
    declared = csim.declared_symbols()
    L = csim.lib()
    for name, nargs in NAMES.items():
        assert name in declared
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    assert csim.OBS_SCREEN_FIELDS == ref.SCREEN_FIELDS and csim.C.sizeof(csim.CsimObsScreenCycle) == 8 * 3
    assert csim.C.sizeof(csim.CsimObsCycle) == 8 * 13   # the first log keeps its thirteen fields
    assert (csim.OBS_USED, csim.OBS_INACTIVE, csim.OBS_REJECTED) == (ref.USED, ref.INACTIVE, ref.REJECTED) == (0, 1, 2)
    for name in ("set_active", "set_reports", "status", "screen_log"):
        assert callable(getattr(csim.ObsNetwork, name))
    assert callable(csim.obs_screen_decide)
    import inspect
    assert inspect.signature(csim.Ensemble.assimilate_network).parameters["screen"].default is None
    header = open(csim.HEADER).read()
    for word in ("CSIM_OBS_USED 0", "CSIM_OBS_INACTIVE 1", "CSIM_OBS_REJECTED 2"):
        assert "#define " + word in header


NAN, INF = float("nan"), float("inf")
BELOW_ONE = float(np.nextafter(1.0, 0.0))

# (y, hb, vb, r, tol, active) -> status, each an edge the header names
EDGES = [
    ((3.0, 1.0, 0.5, 0.5, 2.0, 1), 0),                   # lhs == rhs == 4: equality keeps
    ((3.0, 1.0, BELOW_ONE - 0.5, 0.5, 2.0, 1), 2),       # rhs the next double below 4 = lhs: rejected
    ((float(np.nextafter(3.0, 4.0)), 1.0, 0.5, 0.5, 2.0, 1), 2),
    ((NAN, 1.0, 0.5, 0.5, 2.0, 1), 2),                   # a NaN rejects
    ((3.0, NAN, 0.5, 0.5, 2.0, 1), 2),
    ((3.0, 1.0, NAN, 0.5, 2.0, 1), 2),
    ((NAN, 1.0, 0.5, 0.5, 0.0, 1), 0),                   # tol = 0: never rejected
    ((1e300, -1e300, 0.5, 0.5, 0.0, 1), 0),
    ((1e300, -1e300, 0.5, 0.5, 1e200, 1), 0),            # tol * tol = inf: inf <= inf keeps
    ((3.0, 1.0, 0.0, 1e-300, 1e200, 1), 0),
    ((NAN, 1.0, 0.5, 0.5, 1e200, 1), 2),                 # ... and only a NaN rejects
    ((3.0, 1.0, 0.0, 1.0, 2.0, 1), 0),                   # vb = 0
    ((3.0, 1.0, 0.0, BELOW_ONE, 2.0, 1), 2),
    ((1.0, 1.0, 0.0, 1.0, 1e-200, 1), 0),                # tol > 0 whose square underflows to 0: 0 <= 0 keeps
    ((1.5, 1.0, 0.0, 1.0, 1e-200, 1), 2),
    ((NAN, 1.0, 0.5, 0.5, 2.0, 0), 1),                   # the mask wins over a NaN y
    ((NAN, NAN, NAN, 0.5, 0.0, 0), 1),
    ((3.0, 1.0, 0.5, 0.5, 2.0, 0), 1),
]


@pytest.mark.parametrize("args,want", EDGES)
def test_decide_on_the_named_edges(csim, args, want):
    y, hb, vb, r, tol, active = args
    assert ref.decide(y, hb, vb, r, tol, bool(active)) == want
    assert csim.obs_screen_decide(y, hb, vb, r, tol, active) == want
    assert ref.statuses(np.array([y]), np.array([hb]), np.array([vb]), r, tol, np.array([active]))[0] == want


def test_decide_is_the_restatement(csim):
    """random arguments near the threshold, where one rounding decides: y is put at hb + tol sqrt(vb + r) and moved a few
    units in the last place either way; the products are rounded one by one, so library and restatement agree on all"""
    rng = np.random.default_rng(5)
    n = 4000
    hb, vb, r = rng.standard_normal(n), rng.uniform(0.0, 2.0, n), rng.uniform(0.05, 2.0, n)
    tol = rng.uniform(0.5, 6.0, n)
    y = hb + rng.choice([-1.0, 1.0], n) * tol * np.sqrt(vb + r)
    for step in range(-3, 4):
        yy = y.copy()
        for _ in range(abs(step)):
            yy = np.nextafter(yy, np.where(step > 0, np.inf, -np.inf) * np.sign(yy - hb))
        got = np.array([csim.obs_screen_decide(yy[o], hb[o], vb[o], r[o], tol[o], 1) for o in range(n)])
        want = np.array([ref.decide(yy[o], hb[o], vb[o], r[o], tol[o]) for o in range(n)])
        assert np.array_equal(got, want), step
        assert np.array_equal(want, [ref.statuses(yy[o:o + 1], hb[o:o + 1], vb[o:o + 1], r[o:o + 1], tol[o])[0]
                                     for o in range(n)])
        if step == 0:
            assert 0 < np.count_nonzero(want) < n   # both sides of the threshold occur
    active = rng.integers(0, 2, n)
    got = np.array([csim.obs_screen_decide(y[o], hb[o], vb[o], r[o], 3.0, int(active[o])) for o in range(n)])
    assert np.array_equal(got, ref.statuses(y, hb, vb, r, 3.0, active))


def test_decide_argument_errors(csim):
    L, C = csim.lib(), csim.C
    st = C.c_int(7)
    for tol in (-1.0, -0.5, NAN, INF, -INF):
        assert L.csim_obs_screen_decide(1.0, 0.0, 1.0, 1.0, tol, 1, C.byref(st)) == 1 and st.value == 7
        with pytest.raises(csim.CsimError):
            csim.obs_screen_decide(1.0, 0.0, 1.0, 1.0, tol)
    for active in (2, -1):
        assert L.csim_obs_screen_decide(1.0, 0.0, 1.0, 1.0, 1.0, active, C.byref(st)) == 1 and st.value == 7
    assert L.csim_obs_screen_decide(1.0, 0.0, 1.0, 1.0, 1.0, 1, None) == 1
    assert L.csim_obs_screen_decide(1.0, 0.0, 1.0, 1.0, -0.0, 1, C.byref(st)) == 0 and st.value == 0


def test_null_handles_are_refused_before_the_device(csim):
    L, C = csim.lib(), csim.C
    one = (C.c_ubyte * 1)(1)
    assert L.csim_obs_network_set_active(None, one) == 1 and L.csim_obs_network_set_active(None, None) == 1
    assert L.csim_ensemble_assimilate_screened(None, None, 1.0, -1, 0, 3.0) == 1
    assert L.csim_obs_network_screen_log(None, 0, None, None) == 1
    assert L.csim_obs_network_status(None, one) == 1


@pytest.mark.parametrize("n", [1, 255, 256, 257, 770])
def test_screened_sums_closed_forms(n):
    """dyadic data, every third observation used (k = 3 a, a < m): every partial sum is exact, so each chunked sum with
    +0 terms is the plain sum over the used observations"""
    k = np.arange(n, dtype=np.float64)
    status = np.where(np.arange(n) % 3 == 0, ref.USED, np.where(np.arange(n) % 3 == 1, ref.INACTIVE, ref.REJECTED))
    m = (n + 2) // 3
    S1, S2 = 3 * m * (m - 1) / 2.0, 9 * (m - 1) * m * (2 * m - 1) / 6.0
    y, hb, ha = k / 4.0, k / 8.0, k / 4.0 - 0.5
    y[status != ref.USED] = np.nan   # never looked at
    rec = ref.cycle(y, hb, np.full(n, 2.0), ha, np.full(n, 0.5), 0.25, status, xt=np.where(status == ref.USED, y, 0.0))
    want = dict(n=m, has_truth=1.0, sum_ob=S1 / 8, sum_ob2=S2 / 64, sum_oa=0.5 * m, sum_oa2=0.25 * m,
                sum_oa_ob=S1 / 16, sum_ab_ob=S2 / 64 - S1 / 16, sum_vb=2.0 * m, sum_va=0.5 * m, sum_r=0.25 * m,
                sum_eb2=S2 / 64, sum_ea2=0.25 * m)
    assert set(rec) == set(obsnet.FIELDS)
    for f in obsnet.FIELDS:
        assert rec[f] == want[f], f
    sc = ref.screen_cycle(status)
    assert sc == dict(n_used=m, n_inactive=(n + 1) // 3, n_rejected=n // 3)
    assert sc["n_used"] + sc["n_inactive"] + sc["n_rejected"] == n and sc["n_used"] == rec["n"]
    # nothing used: every sum is +0
    none = ref.cycle(y, hb, np.full(n, 2.0), ha, np.full(n, 0.5), 0.25, np.full(n, ref.INACTIVE))
    assert none["n"] == 0.0 and all(none[f] == 0.0 and not np.signbit(none[f]) for f in obsnet.FIELDS[2:])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 770])
def test_all_used_is_the_unscreened_record(n):
    """a +0 term leaves the bits of a running sum that started from +0: with every observation USED the screened record
    is the csim_obs_cycle of tests/obsnet_restatement.py, and with some not used it is that record of data whose unused
    terms are zeroed"""
    rng = np.random.default_rng(n)
    y, hb, ha, xt = (rng.standard_normal(n) for _ in range(4))
    vb, va, r = rng.uniform(0.1, 2, n), rng.uniform(0.1, 2, n), rng.uniform(0.1, 2, n)
    a = ref.cycle(y, hb, vb, ha, va, r, np.zeros(n, dtype=np.uint8), xt)
    b = obsnet.cycle(y, hb, vb, ha, va, r, xt)
    assert all(np.float64(a[f]).tobytes() == np.float64(b[f]).tobytes() for f in obsnet.FIELDS)
    status = rng.integers(0, 3, n)
    c = ref.cycle(y, hb, vb, ha, va, r, status, xt)
    plain = obsnet.chunked(np.where(status == 0, (y - hb) * (y - hb), 0.0))
    assert np.float64(c["sum_ob2"]).tobytes() == np.float64(plain).tobytes()
    assert c["n"] == np.count_nonzero(status == 0)
