"""Host side of the ensemble-space calls (csim_ensemble_gram, _project, _transform, _eofs, csim_sym_eigen), no GPU
needed: the entry points are declared and exported, the plan of the Gram sum at its seams, the numpy restatement of the
Gram matrix (tests/espace_restatement.py) against an exact reference within its derived bound, the eigensolver through
the library against numpy.linalg.eigh, and the argument errors."""
import numpy as np
import pytest

import espace_restatement as ref
from __graft_entry__ import load_package

NAMES = {"csim_ensemble_gram": 4, "csim_ensemble_gram_plan": 5, "csim_ensemble_project": 6,
         "csim_ensemble_transform": 5, "csim_sym_eigen": 5, "csim_ensemble_eofs": 7, "csim_ensemble_space_check": 6}
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
    assert (csim.ESPACE_MAX_MEMBERS, csim.SYM_EIGEN_MAX_N) == (ref.MAX_MEMBERS, 256)
    assert L.csim_abi_version() == 1


def test_error_codes_are_those_of_the_header(csim):
    txt = " ".join(open(csim.HEADER).read().split())
    assert f"CSIM_ERR_ARG = {ERR_ARG}," in txt and f"CSIM_ERR_UNSUPPORTED = {ERR_UNSUPPORTED}," in txt


# ---- the plan --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,nx,ny,want", [
    (1, 1, 1, (1, 1)), (3, 7, 9, (1, 1)), (3, 8, 8, (1, 1)), (3, 5, 13, (2, 2)), (12, 130, 67, (137, 137)),
    (3, 64, 1024, (1024, 1024)), (3, 64, 1025, (1025, 1024)), (3, 64, 2049, (2049, 1024)),
    (64, 64, 1025, (1025, 1024)), (65, 64, 256, (256, 256)), (65, 64, 257, (257, 256)),
    (128, 64, 257, (257, 256)), (129, 64, 64, (64, 64)), (129, 64, 65, (65, 64)), (256, 64, 65, (65, 64)),
    (64, 1024, 1024, (16384, 1024)),
])
def test_gram_plan_at_the_seams(csim, M, nx, ny, want):
    assert csim.ensemble_gram_plan(M, nx, ny) == want == ref.gram_plan(M, nx, ny)


def test_partial_storage_stays_near_17_mb(csim):
    for M in (64, 128, 256):
        _, Gc = csim.ensemble_gram_plan(M, 4096, 4096)
        assert 16.5e6 < Gc * (M * (M + 1) // 2) * 8 < 17.5e6


# ---- the Gram restatement against the exact reference ----------------------------------------------------------------

@pytest.mark.parametrize("centered", [1, 0])
def test_gram_restatement_within_its_bound_of_the_exact_sum(centered):
    M, nx, ny = 5, 20, 15  # 300 cells: five segments, the last short
    X = ref.members(M, nx, ny, seed=3)
    G = ref.gram(X, None, centered)
    P = ref.interior_rows(ref.perturbations(X, None, centered)[0])
    exact = ref.gram_exact(P)
    bound = ref.gram_bound(P, nx, ny)
    for a in range(M):
        for b in range(M):
            err = abs(float(ref.Fraction(float(G[a, b])) - exact[a][b]))
            assert err <= bound[a, b], (a, b, err, bound[a, b])
    assert np.array_equal(G.view(np.int64), G.T.copy().view(np.int64))


def test_gram_restatement_is_the_plain_sum_where_it_is_exact():
    # small integers: every product and every partial sum is exact, whatever the order
    rng = np.random.default_rng(5)
    X = rng.integers(-8, 9, (4, 11, 30)).astype(np.float64)
    P = ref.interior_rows(X)
    assert np.array_equal(ref.gram(X, None, 0), P @ P.T)
    P3 = ref.interior_rows(X[[0, 1, 3]])
    assert np.array_equal(ref.gram(X, 2, 0), P3 @ P3.T)


def test_project_and_transform_restatements_on_exact_data():
    rng = np.random.default_rng(6)
    X = rng.integers(-8, 9, (4, 5, 6)).astype(np.float64)
    W = rng.integers(-3, 4, (4, 4)).astype(np.float64)
    assert np.array_equal(ref.project(X, W[:, :2], None, 0), np.einsum("kji,kr->rji", X, W[:, :2]))
    sel = np.zeros((4, 4))
    for r, k in enumerate([2, 2, 0, 3]):
        sel[k, r] = 1.0
    Y = ref.transform(X, sel, None, None, 0)
    np.testing.assert_array_equal(Y[:, 1:-1, 1:-1], X[[2, 2, 0, 3]][:, 1:-1, 1:-1])
    ring = np.ones(X.shape[1:], dtype=bool)
    ring[1:-1, 1:-1] = False
    np.testing.assert_array_equal(Y[:, ring], X[:, ring])
    # the identity with a zero shift of the mean keeps centered members up to rounding, the truth member exactly
    Z = ref.transform(X, np.eye(3), np.zeros(3), 1, 1)
    np.testing.assert_array_equal(Z[1], X[1])
    np.testing.assert_allclose(Z, X, rtol=0, atol=1e-14)


# ---- the eigensolver -------------------------------------------------------------------------------------------------

def spd(n, seed):
    rng = np.random.default_rng([seed, n])
    B = rng.standard_normal((n, n + 3))
    return B @ B.T


def eigen_cases():
    cases = {f"spd{n}": spd(n, 1) for n in (1, 2, 3, 17, 64)}
    P = ref.interior_rows(ref.perturbations(ref.members(6, 7, 5, seed=2), None, 1)[0])
    basis = P[:2]
    mix = np.random.default_rng(9).standard_normal((6, 2))
    R = mix @ basis  # six members in a plane: a Gram matrix of rank 2
    cases["rank2"] = R @ R.T
    Q, _ = np.linalg.qr(np.random.default_rng(10).standard_normal((5, 5)))
    cases["repeated"] = (Q * np.array([4.0, 2.0, 2.0, 2.0, 1.0])) @ Q.T
    cases["repeated"] = 0.5 * (cases["repeated"] + cases["repeated"].T)
    cases["diagonal_ties"] = np.diag([1.0, 3.0, 1.0, 3.0])
    return cases


EIGEN = eigen_cases()
FACTOR = 8.0  # Jacobi's other, equally backward-stable path (the issue's allowance over what eigh attains)


def residual(A, lam, V):
    return np.linalg.norm(A @ V - V * lam) / np.linalg.norm(A)


def orthogonality(V):
    return np.linalg.norm(V.T @ V - np.eye(V.shape[0]))


@pytest.mark.parametrize("name", sorted(EIGEN))
def test_sym_eigen_against_eigh(csim, name):
    A = EIGEN[name]
    n = A.shape[0]
    e = csim.sym_eigen(A)
    lam, V = e.lambda_, e.V
    # order and sign rule, exactly
    assert np.all(lam[:-1] >= lam[1:])
    for r in range(n):
        big = int(np.argmax(np.abs(V[:, r])))  # argmax takes the first of equal magnitudes
        assert V[big, r] > 0
    wl, wv = np.linalg.eigh(A)
    wl, wv = wl[::-1], wv[:, ::-1]
    floor = n * 2.0 ** -52
    res, res_ref = residual(A, lam, V), max(residual(A, wl, wv), floor)
    orth, orth_ref = orthogonality(V), max(orthogonality(wv), floor)
    print(f"{name}: sweeps {e.sweeps} residual ratio {res / res_ref:.3f} orthogonality ratio {orth / orth_ref:.3f}")
    assert res <= FACTOR * res_ref
    assert orth <= FACTOR * orth_ref
    assert np.max(np.abs(lam - wl)) <= FACTOR * n * 2.0 ** -52 * np.linalg.norm(A, 2)
    assert 0 <= e.sweeps <= csim.SYM_EIGEN_MAX_SWEEPS


def test_sym_eigen_ties_go_to_the_lower_index_and_only_the_upper_triangle_is_read(csim):
    e = csim.sym_eigen(EIGEN["diagonal_ties"])
    assert e.sweeps == 0 and e.lambda_.tolist() == [3.0, 3.0, 1.0, 1.0]
    assert np.array_equal(e.V, np.eye(4)[:, [1, 3, 0, 2]])
    A = spd(5, 4)
    B = np.triu(A) + np.tril(np.full((5, 5), 7.0), -1)
    a, b = csim.sym_eigen(A), csim.sym_eigen(B)
    assert np.array_equal(a.lambda_.view(np.int64), b.lambda_.view(np.int64))
    assert np.array_equal(a.V.view(np.int64), b.V.view(np.int64))


def test_sym_eigen_is_deterministic(csim):
    A = spd(17, 1)
    a, b = csim.sym_eigen(A), csim.sym_eigen(A.copy())
    assert a.sweeps == b.sweeps and np.array_equal(a.V.view(np.int64), b.V.view(np.int64))


def test_eofs_weights_of_a_rank_2_gram_matrix(csim):
    G = EIGEN["rank2"]
    lam, pcs, W, null = ref.eofs_weights(G, 5, csim.sym_eigen)
    assert null.tolist() == [False, False, True, True, True]
    assert not pcs[:, 2:].any() and not W[:, 2:].any()
    np.testing.assert_allclose(pcs[:, :2] @ pcs[:, :2].T, G, rtol=0, atol=1e-12 * np.linalg.norm(G))


# ---- errors ----------------------------------------------------------------------------------------------------------

def code_of(csim, call):
    with pytest.raises(csim.CsimError) as info:
        call()
    return info.value.code


def test_sym_eigen_errors(csim):
    assert code_of(csim, lambda: csim.sym_eigen(np.empty((0, 0)))) == ERR_ARG
    A = spd(3, 1)
    A[0, 2] = np.nan
    assert code_of(csim, lambda: csim.sym_eigen(A)) == ERR_ARG
    A[0, 2] = np.inf
    assert code_of(csim, lambda: csim.sym_eigen(A)) == ERR_ARG
    assert code_of(csim, lambda: csim.sym_eigen(np.eye(257))) == ERR_UNSUPPORTED
    assert csim.sym_eigen(np.eye(256)).sweeps == 0


def test_argument_errors_without_a_device(csim):
    def check(members, truth_member=None, centered=True, K=0, wbar=False, n_modes=0):
        """csim_ensemble_space_check, the argument checks that gram / project (K) / transform (wbar) / eofs (n_modes)
        of an ensemble of `members` members make; the package has no wrapper for it"""
        rc = csim.lib().csim_ensemble_space_check(members, -1 if truth_member is None else truth_member,
                                                  int(centered), K, int(wbar), n_modes)
        if rc:
            raise csim.CsimError(rc, csim.lib().csim_last_error().decode())

    check(256)
    check(257, truth_member=3)
    check(12, K=12)
    check(12, wbar=True)
    check(12, n_modes=11)
    check(12, truth_member=0, n_modes=10)
    assert code_of(csim, lambda: csim.ensemble_gram_plan(257, 8, 8)) == ERR_UNSUPPORTED
    assert code_of(csim, lambda: csim.ensemble_gram_plan(0, 8, 8)) == ERR_ARG
    assert code_of(csim, lambda: csim.ensemble_gram_plan(3, 0, 8)) == ERR_ARG
    assert code_of(csim, lambda: check(257)) == ERR_UNSUPPORTED            # M > 256
    assert code_of(csim, lambda: check(258, truth_member=0)) == ERR_UNSUPPORTED
    assert code_of(csim, lambda: check(12, K=13)) == ERR_ARG               # K > M
    assert code_of(csim, lambda: check(12, truth_member=0, K=12)) == ERR_ARG
    assert code_of(csim, lambda: check(12, centered=False, wbar=True)) == ERR_ARG
    assert code_of(csim, lambda: check(12, n_modes=12)) == ERR_ARG         # n_modes > M - 1
    assert code_of(csim, lambda: check(12, truth_member=11, n_modes=11)) == ERR_ARG
    assert code_of(csim, lambda: check(12, truth_member=12)) == ERR_ARG
    assert code_of(csim, lambda: check(12, centered=2)) == ERR_ARG
    assert code_of(csim, lambda: check(1, truth_member=0)) == ERR_ARG      # no forecast member
