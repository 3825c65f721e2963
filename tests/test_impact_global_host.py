"""csim_ensemble_dot and csim_ensemble_obs_impact_global without a device: the entry points, the restated dot against an
exact sum and against the restated Gram matrix, and the host-only helper csim_obs_impact_global_value against the
restatement, with its errors."""
import numpy as np
import pytest

import espace_restatement as espace
import impact_global_restatement as ref
from __graft_entry__ import load_package

NAMES = {"csim_ensemble_dot": 6, "csim_ensemble_obs_impact_global": 5, "csim_obs_impact_global_value": 5}
ERR_ARG = 1


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    return pkg


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def test_entry_points_are_declared_and_exported(csim):
    declared = csim.declared_symbols()
    L = csim.lib()
    for name, nargs in NAMES.items():
        assert name in declared
        assert len(getattr(L, name).argtypes) == nargs
    assert csim.DOT_MAX_FIELDS == ref.MAX_FIELDS == 16
    for method in ("dot", "obs_impact_global"):
        assert callable(getattr(csim.Ensemble, method))


# three segments, the last short, one class each; and more segments than the cap of 129 members: classes of two segments
@pytest.mark.parametrize("nx,ny,B,t,centered,K", [(13, 11, 6, 2, 1, 3), (13, 11, 5, None, 0, 1), (65, 64, 130, 0, 1, 2)])
def test_dot_restatement_within_its_bound_of_the_exact_sum(nx, ny, B, t, centered, K):
    X = espace.members(B, nx, ny, seed=3)
    F = np.random.default_rng([5, nx, ny, K]).standard_normal((K, ny + 2, nx + 2))
    got = ref.dot(X, F, t, bool(centered))
    p, _ = espace.perturbations(X, t, bool(centered))
    P, Fi = espace.interior_rows(p), espace.interior_rows(F)
    M = P.shape[0]
    assert got.shape == (M, K)
    rows = list(range(M)) if M < 20 else [0, 64, M - 1]      # the exact sums of a few members are enough at 4160 cells
    exact = ref.dot_exact(P[rows], Fi)
    bound = ref.dot_bound(P[rows], Fi, nx, ny, M)
    for a, k in enumerate(rows):
        for r in range(K):
            err = abs(float(ref.Fraction(float(got[k, r])) - exact[a][r]))
            assert err <= bound[a, r], (k, r, err, bound[a, r])


@pytest.mark.parametrize("nx,ny,B,t", [(9, 7, 5, None), (13, 11, 6, 3), (65, 64, 66, 65), (33, 64, 130, 0)])
def test_dot_of_member_fields_is_the_gram_matrix(nx, ny, B, t):
    """centered = 0 and f_r the field of forecast member b: the same products in the same order, so gram's bits"""
    X = espace.members(B, nx, ny, seed=7)
    fc = espace.forecast(B, t)
    G = espace.gram(X, t, centered=False)
    for b0 in range(0, len(fc), ref.MAX_FIELDS):
        cols = fc[b0:b0 + ref.MAX_FIELDS]
        got = ref.dot(X, X[cols], t, centered=False)
        assert np.array_equal(bits(got), bits(G[:, b0:b0 + len(cols)]))
        if b0 >= 2 * ref.MAX_FIELDS:
            break


def test_dot_restatement_ignores_ghosts_and_the_truth_member():
    nx, ny, B, t = 13, 5, 4, 1
    X = espace.members(B, nx, ny, seed=1)
    F = np.random.default_rng(2).standard_normal((2, ny + 2, nx + 2))
    want = ref.dot(X, F, t, True)
    Xn, Fn = X.copy(), F.copy()
    Xn[t] = np.nan
    for A in (Xn, Fn):
        A[:, 0, :] = A[:, -1, :] = A[:, :, 0] = A[:, :, -1] = np.nan
    assert np.array_equal(bits(ref.dot(Xn, Fn, t, True)), bits(want))


@pytest.mark.parametrize("M", [2, 3, 64, 65, 256])
def test_value_is_the_restatement(csim, M):
    rng = np.random.default_rng(M)
    a, g = rng.standard_normal(M), 1e-3 * rng.standard_normal(M)
    for dn in (1.75, -0.3, 0.0, -0.0):
        got = csim.obs_impact_global_value(a, g, dn)
        assert bits(got) == bits(ref.value(a, g, dn)), (M, dn)
    assert bits(csim.obs_impact_global_value(a, np.zeros(M), 2.0)) == 0      # +0, not -0


def test_value_is_not_a_pairwise_or_contracted_sum(csim):
    """terms whose running sum in member order differs from their sum in another order or with fused products"""
    a = np.array([1.0, 2.0 ** -53, 2.0 ** -53, -1.0])
    g = np.ones(4)
    assert csim.obs_impact_global_value(a, g, 3.0) == ref.value(a, g, 3.0) == 0.0
    assert csim.obs_impact_global_value(a[::-1].copy(), g, 3.0) != 0.0


def test_value_errors(csim):
    L, C = csim.lib(), csim.C
    a = np.ones(3)
    ap = a.ctypes.data_as(C.POINTER(C.c_double))
    out = C.c_double(7.0)
    for M in (1, 0, -4):
        assert L.csim_obs_impact_global_value(M, ap, ap, 1.0, C.byref(out)) == ERR_ARG
    assert L.csim_obs_impact_global_value(3, None, ap, 1.0, C.byref(out)) == ERR_ARG
    assert L.csim_obs_impact_global_value(3, ap, None, 1.0, C.byref(out)) == ERR_ARG
    assert L.csim_obs_impact_global_value(3, ap, ap, 1.0, None) == ERR_ARG
    assert out.value == 7.0
    assert L.csim_obs_impact_global_value(3, ap, ap, 2.0, C.byref(out)) == 0 and out.value == 3.0
    with pytest.raises(ValueError):
        csim.obs_impact_global_value(np.ones(3), np.ones(4), 1.0)


def test_dot_checks_need_no_device(csim):
    """a null ensemble is refused before anything else"""
    L = csim.lib()
    assert L.csim_ensemble_dot(None, -1, 1, 1, None, None) == ERR_ARG
    assert L.csim_ensemble_obs_impact_global(None, None, None, None, None) == ERR_ARG
