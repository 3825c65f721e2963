"""Host side of the per-observation forecast impact (csim_obs_network_impact_capture, csim_ensemble_obs_impact,
csim_obs_impact_fold in include/csim.h), no GPU needed: the entry points are declared and exported, csim_obs_impact_fold
is the restatement's fold (tests/impact_restatement.py) bit for bit on sums whose order shows in the bits, impact_weight
is its formula, and the argument errors that need no device are refused."""
import numpy as np
import pytest

import impact_restatement as ref
from __graft_entry__ import load_package

NAMES = {"csim_obs_network_impact_capture": 2, "csim_ensemble_obs_impact": 5, "csim_obs_impact_fold": 3}


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    return pkg


def bits(v):
    return np.float64(v).tobytes()


def test_entry_points_are_declared_and_exported(csim):
    declared = csim.declared_symbols()
    L = csim.lib()
    for name, nargs in NAMES.items():
        assert name in declared
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    assert csim.C.sizeof(csim.CsimObsImpactSummary) == 24
    assert csim.ObsImpactSummary._fields == ("used", "beneficial", "total") and csim.ObsImpact._fields == ("impact", "summary")
    assert callable(csim.ObsNetwork.impact_capture) and callable(csim.Ensemble.obs_impact)
    assert callable(csim.impact_weight) and callable(csim.obs_impact_fold)
    header = open(csim.HEADER).read()
    assert "#define CSIM_IMPACT_MAX_DOUBLES (1L << 27)" in header and csim.IMPACT_MAX_DOUBLES == 1 << 27
    assert csim.IMPACT_MAX_DOUBLES * 8 <= 1 << 30          # the perturbations stay at or below 1 GiB
    assert "#define CSIM_ABI_VERSION 1" in header and L.csim_abi_version() == 1


def mixed(rng, n):
    """mixed signs and magnitudes over thirty binades: every addition rounds, so the order of a sum shows in its bits"""
    return rng.standard_normal(n) * np.exp2(rng.integers(-15, 16, n).astype(np.float64))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129, 300, 777])
def test_fold_is_the_restatement(csim, n):
    differs = 0
    for seed in range(8):
        u = mixed(np.random.default_rng(1000 * n + seed), n)
        got, want = csim.obs_impact_fold(u), ref.fold(u)
        assert bits(got) == bits(want), (n, seed, got, want)
        differs += bits(want) != bits(ref.plain_sum(u))
        # both are sums of the same n terms: each is within (n - 1) 2^-53 sum |u| of the exact one, to first order
        assert abs(want - ref.plain_sum(u)) <= n * 2.0 ** -51 * np.abs(u).sum()
    # with three terms or more the lane order is another order than the plain one, and on this data it shows
    if n >= 63:
        assert differs > 0, "the data must tell the fold from a running sum"
    if n <= 1:
        assert differs == 0
    if n == 0:
        assert bits(csim.obs_impact_fold([])) == bits(0.0)


def test_fold_order_on_a_hand_made_case(csim):
    """1 + 2^-53 + 2^-53: a running sum that meets 1 first loses both small terms (ties to even); where the two small
    terms meet first they survive.  Terms 0, 64 and 128 all go to lane 0; lanes 1 and 3 meet at h = 2, before lane 0"""
    t = 2.0 ** -53
    u = np.zeros(129)
    u[0], u[64], u[128] = t, t, 1.0          # lane 0: (t + t) + 1 = 1 + 2^-52
    assert csim.obs_impact_fold(u) == 1.0 + 2.0 ** -52 == ref.fold(u)
    x = np.zeros(4)
    x[0], x[1], x[3] = 1.0, t, t             # h = 2: l[1] = l[1] + l[3] = 2^-52; h = 1: l[0] = 1 + 2^-52; plain: 1
    assert csim.obs_impact_fold(x) == ref.fold(x) == 1.0 + 2.0 ** -52 != ref.plain_sum(x)
    # signed zeros and non-finite terms pass through the adds
    assert bits(csim.obs_impact_fold([-0.0])) == bits(ref.fold([-0.0])) == bits(0.0)
    assert np.isnan(csim.obs_impact_fold([np.inf, -np.inf])) and np.isnan(ref.fold([np.inf, -np.inf]))
    assert csim.obs_impact_fold([np.inf] + [0.0] * 63 + [np.inf]) == np.inf


def test_fold_argument_errors(csim):
    L, C = csim.lib(), csim.C
    out = C.c_double(7.0)
    one = (C.c_double * 1)(1.0)
    assert L.csim_obs_impact_fold(one, -1, C.byref(out)) == 1 and out.value == 7.0
    assert L.csim_obs_impact_fold(None, 1, C.byref(out)) == 1 and out.value == 7.0
    assert L.csim_obs_impact_fold(one, 1, None) == 1
    assert L.csim_obs_impact_fold(None, 0, C.byref(out)) == 0 and bits(out.value) == bits(0.0)
    with pytest.raises(ValueError):
        csim.obs_impact_fold(np.zeros((2, 2)))


def test_null_handles_are_refused_before_the_device(csim):
    L, C = csim.lib(), csim.C
    w = (C.c_double * 9)()
    out = (C.c_double * 1)()
    sm = csim.CsimObsImpactSummary()
    assert L.csim_obs_network_impact_capture(None, -1) == 1
    assert L.csim_ensemble_obs_impact(None, None, w, out, C.byref(sm)) == 1
    assert b"null" in L.csim_last_error()


def test_impact_weight_is_its_formula(csim):
    rng = np.random.default_rng(3)
    ny, nx = 17, 33
    a, b, t = (rng.standard_normal((ny + 2, nx + 2)) for _ in range(3))
    w = csim.impact_weight(a, b, t)
    want = ref.impact_weight(a, b, t)
    assert w.shape == (ny + 2, nx + 2) and w.dtype == np.float64 and w.tobytes() == want.tobytes()
    ring = np.ones(w.shape, dtype=bool)
    ring[1:-1, 1:-1] = False
    assert not w[ring].any() and not np.signbit(w[ring]).any()
    j, i = 5, 7
    assert w[j, i] == ((a[j, i] - t[j, i]) + (b[j, i] - t[j, i])) / (nx * ny)
    # sum w (e_a - e_b) is e_a' C e_a - e_b' C e_b for C = I / (nx ny): the mean squared errors' difference
    ea, eb = (a - t)[1:-1, 1:-1], (b - t)[1:-1, 1:-1]
    assert np.isclose((w[1:-1, 1:-1] * (ea - eb)).sum(), (ea ** 2).mean() - (eb ** 2).mean(), rtol=1e-12, atol=1e-15)
    for bad in ((a, b, t[1:]), (a[0], b[0], t[0]), (a[:2], b[:2], t[:2])):
        with pytest.raises(ValueError):
            csim.impact_weight(*bad)


def test_restatement_window_terms_by_hand():
    """two members, one observation in a corner, a table with a zero: the terms are (rho (c / (M-1))) w in window order
    and +0 under rho == 0, whatever the cell holds"""
    X = np.zeros((2, 5, 6))
    X[0, 1:-1, 1:-1] = np.arange(12.0).reshape(3, 4)
    X[1, 1:-1, 1:-1] = -np.arange(12.0).reshape(3, 4)
    X[0, 2, 2] = np.nan                                  # under rho == 0
    rho = np.array([[0.25, 0.5, 0.25], [0.5, 1.0, 0.5], [0.25, 0.5, 0.0]])
    w = np.full((5, 6), 2.0)
    cap = ref.capture(X, None, np.array([1]), np.array([1]), None, np.array([3.0]), np.array([1.0]), 0.5)
    assert cap.a.tolist() == [[0.0, 0.0]] and cap.dn.tolist() == [4.0] and cap.status.tolist() == [0]
    cap = cap._replace(a=np.array([[1.0, -1.0]]))
    u = ref.terms(X, cap, rho, 1, 1, cap.a[0], w)        # window (1..2) x (1..2): cells 0, 1, 4, (5 = NaN cell)
    # xbar = 0, c = 2 x_0 = 0, 2, 8 and NaN; rho = 1, 0.5, 0.5 and 0; w = 2
    assert u.tolist() == [0.0, 2.0, 8.0, 0.0]
    J = ref.impact(X, cap, rho, np.array([1]), np.array([1]), w)
    assert J.tolist() == [4.0 * 10.0] and ref.summary(J, cap.status) == (1, 0, 40.0)
    unused = cap._replace(status=np.array([2], dtype=np.uint8))
    J = ref.impact(X, unused, rho, np.array([1]), np.array([1]), w)
    assert bits(J[0]) == bits(0.0) and ref.summary(J, unused.status) == (0, 0, 0.0)
