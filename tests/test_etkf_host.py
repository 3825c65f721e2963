"""Host side of the ETKF (csim_ensemble_obs_gram, csim_obs_gram_plan, csim_etkf_weights, csim_ensemble_assimilate_etkf),
no GPU needed: the entry points are declared and exported, the plan of the observation-space Gram sum at its seams, the
numpy restatement of the matrix (tests/etkf_restatement.py) against an exact reference within its derived bound, the
weights through the library against the restatement bit for bit and against the dense Kalman update, and the errors.

Only the two tests that pin the restatement of the matrix (..._within_its_bound_of_the_exact_sum and
..._is_the_plain_sum_where_it_is_exact) run without the library's new symbols."""
import numpy as np
import pytest

import etkf_restatement as ref
from __graft_entry__ import load_package

NAMES = {"csim_ensemble_obs_gram": 6, "csim_obs_gram_plan": 4, "csim_etkf_weights": 8,
         "csim_ensemble_assimilate_etkf": 6, "csim_ensemble_etkf_info": 6}
ERR_ARG, ERR_UNSUPPORTED = 1, 5


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
        assert len(getattr(L, name).argtypes) == nargs
    assert csim.ESPACE_MAX_MEMBERS == ref.MAX_MEMBERS


# ---- the plan --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,nobs,want", [
    (2, 1, (1, 1)), (8, 63, (1, 1)), (8, 64, (1, 1)), (8, 65, (2, 2)), (8, 65536, (1024, 1024)),
    (8, 65537, (1025, 1024)), (64, 65537, (1025, 1024)), (65, 16384, (256, 256)), (65, 16385, (257, 256)),
    (128, 16385, (257, 256)), (129, 4096, (64, 64)), (129, 4097, (65, 64)), (256, 4097, (65, 64)),
    (256, 1 << 20, (16384, 64)),
])
def test_obs_gram_plan_at_the_seams(csim, M, nobs, want):
    assert csim.obs_gram_plan(M, nobs) == want == ref.gram_plan(M, nobs)


# ---- the restatement of the matrix against the exact reference -------------------------------------------------------

def observations(M, nobs, seed, masked=()):
    rng = np.random.default_rng([seed, M, nobs])
    H = 3.0 + rng.standard_normal((M, nobs))
    y = 3.0 + rng.standard_normal(nobs)
    r = rng.uniform(0.5, 2.0, nobs)
    used = np.ones(nobs, dtype=bool)
    used[list(masked)] = False
    return H, y, r, used


def test_obs_gram_restatement_within_its_bound_of_the_exact_sum():
    M, nobs = 5, 300  # five segments, the last short; a shuffled plan order; three observations masked
    H, y, r, used = observations(M, nobs, 3, masked=(0, 77, 299))
    order = np.random.default_rng(4).permutation(nobs)
    A, ll, n_used = ref.obs_gram(H, y, r, used, order, loglik=True)
    assert n_used == nobs - 3
    Z, E = ref.rows(H, y, r, used, order)
    assert not Z[np.isin(order, (0, 77, 299))].any()
    exact, bound = ref.gram_exact(Z), ref.gram_bound(Z, M)
    for a in range(M + 1):
        for b in range(M + 1):
            err = abs(float(ref.Fraction(float(A[a, b])) - exact[a][b]))
            assert err <= bound[a, b], (a, b, err, bound[a, b])
    assert np.array_equal(A.view(np.int64), A.T.copy().view(np.int64))
    exact_e, bound_e = ref.gram_exact(E), ref.gram_bound(E, M)
    for k in range(M):
        assert abs(float(ref.Fraction(float(ll[k])) - exact_e[k][k])) <= bound_e[k, k]


def test_obs_gram_restatement_is_the_plain_sum_where_it_is_exact():
    # small integers, r = 1 or 4 and a member mean that is an integer: every operation is exact, whatever the order
    rng = np.random.default_rng(5)
    M, nobs = 4, 150
    H = rng.integers(-8, 9, (M, nobs)).astype(np.float64)
    H[0] -= H.sum(axis=0) % M
    y = rng.integers(-8, 9, nobs).astype(np.float64)
    r = rng.choice([1.0, 4.0], nobs)
    used = rng.random(nobs) < 0.8
    order = rng.permutation(nobs)
    A, ll, n_used = ref.obs_gram(H, y, r, used, order, loglik=True)
    Z = np.vstack([H - H.mean(axis=0), (y - H.mean(axis=0))[None]]) / np.sqrt(r) * used
    assert np.array_equal(A, Z @ Z.T)
    assert np.array_equal(ll, ((((y - H) / np.sqrt(r)) * used) ** 2).sum(axis=1))
    assert n_used == used.sum()


# ---- the weights -----------------------------------------------------------------------------------------------------

def gram_of(M, nobs, seed):
    H, y, r, used = observations(M, nobs, seed)
    return ref.obs_gram(H, y, r, used, np.arange(nobs))[0], (H, y, r)


@pytest.mark.parametrize("M,nobs,inflation", [(2, 1, 1.0), (3, 40, 1.1), (16, 40, 1.0), (16, 7, 1.5), (65, 100, 1.1)])
def test_etkf_weights_are_the_restatement(csim, M, nobs, inflation):
    A, _ = gram_of(M, nobs, 11)
    got = csim.etkf_weights(A, inflation)
    W, wbar, gamma, dfs, sweeps = ref.etkf_weights(A, inflation, csim.sym_eigen)
    for g, w in ((got.W, W), (got.wbar, wbar), (got.gamma, gamma), (np.float64(got.dfs), np.float64(dfs))):
        assert np.array_equal(np.asarray(g).view(np.int64), np.asarray(w).view(np.int64))
    assert got.sweeps == sweeps
    assert np.array_equal(got.W.view(np.int64), got.W.T.copy().view(np.int64))
    assert np.all(got.gamma >= 0) and 0 <= got.dfs <= min(M - 1, nobs) + 1e-9
    # the ensemble mean of the perturbations stays zero: W 1 = inflation 1 (C 1 = 0 up to rounding)
    np.testing.assert_allclose(got.W.sum(axis=1), inflation, rtol=0, atol=1e-12 * M)


def test_etkf_weights_without_observations_only_inflate(csim):
    M = 6
    for inflation in (1.0, 1.25):
        got = csim.etkf_weights(np.zeros((M + 1, M + 1)), inflation)
        np.testing.assert_allclose(got.W, inflation * np.eye(M), rtol=0, atol=4e-16)
        assert not got.wbar.any() and not got.gamma.any() and got.dfs == 0.0 and got.sweeps == 0


def test_etkf_weights_outputs_are_optional(csim):
    A, _ = gram_of(4, 9, 2)
    a = np.ascontiguousarray(A)
    none = [None] * 5
    assert csim.lib().csim_etkf_weights(4, a.ctypes.data_as(csim.C.POINTER(csim.C.c_double)), 1.0, *none) == 0


FACTOR = 8.0  # what tests/test_espace_host.py grants sym_eigen over eigh


@pytest.mark.parametrize("inflation", [1.0, 1.1])
@pytest.mark.parametrize("M,nobs", [(2, 5), (5, 40), (16, 40), (16, 9), (9, 1)])
def test_etkf_weights_against_the_dense_kalman_update(csim, M, nobs, inflation):
    A, (H, y, r) = gram_of(M, nobs, 21)
    got = csim.etkf_weights(A, inflation)
    mine = ref.kalman_distance(H, y, r, inflation, got.W, got.wbar)
    yard = ref.kalman_distance(H, y, r, inflation, *ref.etkf_eigh(H, y, r, inflation))
    print(f"M {M} nobs {nobs} inflation {inflation}: distance {mine:.3e}, eigh {yard:.3e}, ratio {mine / yard:.3f}")
    assert mine <= FACTOR * yard


# ---- errors ----------------------------------------------------------------------------------------------------------

def code_of(csim, call):
    with pytest.raises(csim.CsimError) as info:
        call()
    return info.value.code


def test_argument_errors_without_a_device(csim):
    A, _ = gram_of(3, 5, 1)
    assert code_of(csim, lambda: csim.etkf_weights(np.zeros((2, 2)))) == ERR_ARG          # M = 1
    assert code_of(csim, lambda: csim.etkf_weights(np.zeros((258, 258)))) == ERR_UNSUPPORTED
    assert csim.etkf_weights(np.zeros((257, 257))).sweeps == 0
    for bad in (0.999, -1.0, np.nan, np.inf):
        assert code_of(csim, lambda: csim.etkf_weights(A, bad)) == ERR_ARG
    for where in ((0, 1), (3, 3), (1, 3), (3, 0)):
        for v in (np.nan, np.inf):
            B = A.copy()
            B[where] = v
            assert code_of(csim, lambda: csim.etkf_weights(B)) == ERR_ARG
    assert code_of(csim, lambda: csim.obs_gram_plan(1, 5)) == ERR_ARG
    assert code_of(csim, lambda: csim.obs_gram_plan(3, 0)) == ERR_ARG
    assert code_of(csim, lambda: csim.obs_gram_plan(257, 5)) == ERR_UNSUPPORTED
