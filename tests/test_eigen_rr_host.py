"""Host side of the round-robin Jacobi order (csim_sym_eigen_ordered, csim_etkf_weights_ordered,
csim_sym_eigen_device_form), no GPU needed: the library against the numpy restatement of the order
(tests/eigen_rr_restatement.py) bit for bit, order 0 against csim_sym_eigen bit for bit, the symmetry of the working
matrix after every step, the accuracy against numpy.linalg.eigh with the yardstick of tests/test_espace_host.py, the
weights on top of the order against the restatement and the dense Kalman update, and the errors.

Only test_pairing_takes_every_pair_once_per_sweep and test_restatement_keeps_a_symmetric_after_every_step run without
the library's new symbols: they pin the restatement alone."""
import numpy as np
import pytest

import eigen_rr_restatement as rr
import etkf_restatement as etkf
from __graft_entry__ import load_package

NAMES = {"csim_sym_eigen_ordered": 6, "csim_sym_eigen_batch_gpu": 8, "csim_sym_eigen_device_form": 4,
         "csim_etkf_weights_ordered": 9, "csim_ensemble_assimilate_etkf_device": 6, "csim_ensemble_etkf_info2": 8}
ERR_ARG, ERR_UNSUPPORTED = 1, 5
FACTOR = 8.0  # the allowance of tests/test_espace_host.py over what eigh attains on the same matrix


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    return pkg


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def gram(n, seed, rank=None):
    rng = np.random.default_rng([seed, n])
    B = rng.standard_normal((n, (n + 3) if rank is None else rank))
    return B @ B.T


def cases():
    out = {f"gram{n}": gram(n, 1) for n in (1, 2, 3, 4, 5, 8, 63, 64, 65)}
    out["diagonal"] = np.diag([2.0, -1.0, 5.0, 5.0, 0.0])
    E = np.full((6, 6), 0.25) + np.eye(6) * 3.0          # equal diagonals: theta = 0 in every first rotation
    out["equal_diagonals"] = E
    u = np.random.default_rng(3).standard_normal(7)
    out["rank1"] = np.outer(u, u)
    sc = np.array([1e150, 1.0, 1e-150, 1e75, 1e-75, 3.0])  # a_pq / h where h dwarfs a_pq, and the tiny test
    S = np.random.default_rng(4).standard_normal((6, 6))
    S = (S + S.T) * np.sqrt(np.outer(sc, sc))
    S[np.diag_indices(6)] = sc
    out["scales"] = S
    out["negative_definite"] = -gram(9, 5)
    return out


CASES = cases()


def test_entry_points_and_constants(csim):
    declared = csim.declared_symbols()
    L = csim.lib()
    for name, nargs in NAMES.items():
        assert name in declared
        assert len(getattr(L, name).argtypes) == nargs
    txt = " ".join(open(csim.HEADER).read().split())
    assert "#define CSIM_EIGEN_ROWS 0" in txt and "#define CSIM_EIGEN_ROUND_ROBIN 1" in txt
    assert csim.EIGEN_ORDERS == {"rows": 0, "round_robin": 1}
    assert rr.MAX_SWEEPS == csim.SYM_EIGEN_MAX_SWEEPS


@pytest.mark.parametrize("n", list(range(1, 67)) + [255, 256])
def test_pairing_takes_every_pair_once_per_sweep(n):
    m = n + (n & 1)
    seen = np.zeros((m, m), dtype=int)
    for t in range(m - 1):
        p, q = rr.pairs(n, t)
        assert len(p) == m // 2 and np.all(p < q) and np.all(q < m)
        assert len(set(p.tolist()) | set(q.tolist())) == m  # the slots of a step are disjoint
        if n & 1:
            assert q[0] == n and p[0] == t and np.all(q[1:] < n)  # the idle slot is slot 0, its lone index t
        seen[p, q] += 1
    assert np.array_equal(seen, np.triu(np.ones((m, m), dtype=int), 1))


@pytest.mark.parametrize("name", ["gram5", "gram8", "scales", "rank1"])
def test_restatement_keeps_a_symmetric_after_every_step(name):
    steps = []

    def symmetric(a):
        steps.append(1)
        assert np.array_equal(bits(a), bits(a.T))

    rr.sym_eigen_rr(CASES[name], symmetric)
    assert steps


@pytest.mark.parametrize("name", sorted(CASES))
def test_round_robin_is_the_restatement_bit_for_bit(csim, name):
    A = CASES[name]
    got = csim.sym_eigen(A, order="round_robin")
    lam, V, sweeps = rr.sym_eigen_rr(A)
    assert got.sweeps == sweeps
    assert np.array_equal(bits(got.lambda_), bits(lam))
    assert np.array_equal(bits(got.V), bits(V))
    if name == "diagonal":
        assert sweeps == 0 and got.lambda_.tolist() == [5.0, 5.0, 2.0, 0.0, -1.0]
        assert np.array_equal(got.V, np.eye(5)[:, [2, 3, 0, 4, 1]])


def test_only_the_upper_triangle_is_read(csim):
    A = gram(6, 7)
    B = np.triu(A) + np.tril(np.full((6, 6), 7.0), -1)
    a, b = csim.sym_eigen(A, order="round_robin"), csim.sym_eigen(B, order="round_robin")
    assert np.array_equal(bits(a.lambda_), bits(b.lambda_)) and np.array_equal(bits(a.V), bits(b.V))


@pytest.mark.parametrize("name", sorted(CASES))
def test_order_0_is_sym_eigen_bit_for_bit(csim, name):
    A = CASES[name]
    n = A.shape[0]
    lam, V, sweeps = np.empty(n), np.empty((n, n)), csim.C.c_int()
    dp = lambda a: a.ctypes.data_as(csim.C.POINTER(csim.C.c_double))
    a = np.ascontiguousarray(A)
    assert csim.lib().csim_sym_eigen(n, dp(a), dp(lam), dp(V), csim.C.byref(sweeps)) == 0
    for got in (csim.sym_eigen(A), csim.sym_eigen(A, order="rows"), csim.sym_eigen(A, order=0)):
        assert got.sweeps == sweeps.value
        assert np.array_equal(bits(got.lambda_), bits(lam)) and np.array_equal(bits(got.V), bits(V))


# ---- accuracy: the yardstick of tests/test_espace_host.py, on its matrices and at n = 128 ------------------------------

def eigh_cases():
    import test_espace_host as espace
    out = dict(espace.EIGEN)
    out["gram128"] = gram(128, 2)
    out["gram128_rank32"] = gram(128, 2, rank=32)
    return out


EIGH = eigh_cases()


def residual(A, lam, V):
    return np.linalg.norm(A @ V - V * lam) / np.linalg.norm(A)


def orthogonality(V):
    return np.linalg.norm(V.T @ V - np.eye(V.shape[0]))


@pytest.mark.parametrize("name", sorted(EIGH))
def test_round_robin_against_eigh(csim, name):
    """Attained on this yardstick (ratio to what eigh attains on the same matrix, floor n 2^-52): the figures are
    printed; every matrix stays within FACTOR = 8, so the wider allowance of 4 x the row order is not drawn on."""
    A = EIGH[name]
    n = A.shape[0]
    e = csim.sym_eigen(A, order="round_robin")
    lam, V = e.lambda_, e.V
    assert np.all(lam[:-1] >= lam[1:])
    for r in range(n):
        assert V[int(np.argmax(np.abs(V[:, r]))), r] > 0
    wl, wv = np.linalg.eigh(A)
    wl, wv = wl[::-1], wv[:, ::-1]
    floor = n * 2.0 ** -52
    res, res_ref = residual(A, lam, V), max(residual(A, wl, wv), floor)
    orth, orth_ref = orthogonality(V), max(orthogonality(wv), floor)
    rows = csim.sym_eigen(A)
    print(f"{name}: sweeps {e.sweeps} (rows {rows.sweeps}) residual ratio {res / res_ref:.3f} "
          f"(rows {residual(A, rows.lambda_, rows.V) / res_ref:.3f}) orthogonality ratio {orth / orth_ref:.3f} "
          f"(rows {orthogonality(rows.V) / orth_ref:.3f})")
    assert res <= FACTOR * res_ref
    assert orth <= FACTOR * orth_ref
    assert np.max(np.abs(lam - wl)) <= FACTOR * n * 2.0 ** -52 * np.linalg.norm(A, 2)
    assert 0 <= e.sweeps < csim.SYM_EIGEN_MAX_SWEEPS


# ---- the weights on top of the order -----------------------------------------------------------------------------------

def observations(M, nobs, seed):
    rng = np.random.default_rng([seed, M, nobs])
    H = 3.0 + rng.standard_normal((M, nobs))
    y = 3.0 + rng.standard_normal(nobs)
    r = rng.uniform(0.5, 2.0, nobs)
    return H, y, r


def gram_of(M, nobs, seed):
    H, y, r = observations(M, nobs, seed)
    return etkf.obs_gram(H, y, r, np.ones(nobs, dtype=bool), np.arange(nobs))[0], (H, y, r)


@pytest.mark.parametrize("M,nobs,inflation", [(2, 1, 1.0), (3, 40, 1.1), (16, 40, 1.0), (16, 7, 1.5), (65, 100, 1.1)])
def test_etkf_weights_round_robin_are_the_restatement(csim, M, nobs, inflation):
    A, _ = gram_of(M, nobs, 11)
    got = csim.etkf_weights(A, inflation, order="round_robin")
    W, wbar, gamma, dfs, sweeps = etkf.etkf_weights(A, inflation, lambda C: csim.SymEigen(*rr.sym_eigen_rr(C)))
    for g, w in ((got.W, W), (got.wbar, wbar), (got.gamma, gamma), (np.float64(got.dfs), np.float64(dfs))):
        assert np.array_equal(bits(g), bits(w))
    assert got.sweeps == sweeps
    assert np.array_equal(bits(got.W), bits(got.W.T.copy()))  # symmetric bit for bit
    rows = csim.etkf_weights(A, inflation)
    ordered0 = csim.etkf_weights(A, inflation, order="rows")
    assert np.array_equal(bits(rows.W), bits(ordered0.W)) and np.array_equal(bits(rows.wbar), bits(ordered0.wbar))
    np.testing.assert_allclose(got.W, rows.W, rtol=0, atol=1e-12)


@pytest.mark.parametrize("inflation", [1.0, 1.1])
@pytest.mark.parametrize("M,nobs", [(2, 5), (5, 40), (16, 40), (16, 9), (9, 1)])
def test_etkf_weights_round_robin_against_the_dense_kalman_update(csim, M, nobs, inflation):
    """the Kalman check of tests/test_etkf_host.py with its allowance, 8 x the distance of the eigh ETKF; the attained
    ratios are printed"""
    A, (H, y, r) = gram_of(M, nobs, 21)
    got = csim.etkf_weights(A, inflation, order="round_robin")
    mine = etkf.kalman_distance(H, y, r, inflation, got.W, got.wbar)
    yard = etkf.kalman_distance(H, y, r, inflation, *etkf.etkf_eigh(H, y, r, inflation))
    print(f"M {M} nobs {nobs} inflation {inflation}: distance {mine:.3e}, eigh {yard:.3e}, ratio {mine / yard:.3f}")
    assert mine <= FACTOR * yard


# ---- the device forms, without a device --------------------------------------------------------------------------------

def test_device_forms_and_their_boundaries(csim):
    assert csim.sym_eigen_device_form(1) == (1, 256)
    b1, b2 = csim.sym_eigen_device_form(1, 1)[1], csim.sym_eigen_device_form(1, 2)[1]
    assert 1 < b1 < b2 < 256 and csim.sym_eigen_device_form(1, 3)[1] == 256
    assert 16 * b1 * b1 <= 156 * 1024 and 8 * b2 * b2 <= 156 * 1024  # they fit the LDS beside the slots' parameters
    for n, want in ((b1, 1), (b1 + 1, 2), (b2, 2), (b2 + 1, 3), (256, 3)):
        assert csim.sym_eigen_device_form(n)[0] == want
    for form, most in ((1, b1), (2, b2), (3, 256)):
        assert csim.sym_eigen_device_form(most, form)[0] == form
        assert csim.sym_eigen_device_form(5, form)[0] == form


# ---- errors ------------------------------------------------------------------------------------------------------------

def code_of(csim, call):
    with pytest.raises(csim.CsimError) as info:
        call()
    return info.value.code


def test_argument_errors_and_non_finite_input(csim):
    A = gram(3, 1)
    assert code_of(csim, lambda: csim.sym_eigen(A, order=2)) == ERR_ARG
    assert code_of(csim, lambda: csim.sym_eigen(A, order=-1)) == ERR_ARG
    assert code_of(csim, lambda: csim.sym_eigen(np.empty((0, 0)), order="round_robin")) == ERR_ARG
    assert code_of(csim, lambda: csim.sym_eigen(np.eye(257), order="round_robin")) == ERR_UNSUPPORTED
    assert csim.sym_eigen(np.eye(256), order="round_robin").sweeps == 0
    for v in (np.nan, np.inf, -np.inf):
        for where in ((0, 2), (2, 0), (1, 1)):
            B = A.copy()
            B[where] = v
            assert code_of(csim, lambda: csim.sym_eigen(B, order="round_robin")) == ERR_ARG
    G, _ = gram_of(3, 5, 1)
    assert code_of(csim, lambda: csim.etkf_weights(G, 1.0, order=2)) == ERR_ARG
    assert code_of(csim, lambda: csim.etkf_weights(np.zeros((2, 2)), order="round_robin")) == ERR_ARG
    assert code_of(csim, lambda: csim.etkf_weights(np.zeros((258, 258)), order="round_robin")) == ERR_UNSUPPORTED
    assert code_of(csim, lambda: csim.etkf_weights(G, 0.5, order="round_robin")) == ERR_ARG
    B = G.copy()
    B[1, 3] = np.nan
    assert code_of(csim, lambda: csim.etkf_weights(B, order="round_robin")) == ERR_ARG
    assert code_of(csim, lambda: csim.sym_eigen_device_form(0)) == ERR_ARG
    assert code_of(csim, lambda: csim.sym_eigen_device_form(5, 4)) == ERR_ARG
    assert code_of(csim, lambda: csim.sym_eigen_device_form(257)) == ERR_UNSUPPORTED
    b1 = csim.sym_eigen_device_form(1, 1)[1]
    assert code_of(csim, lambda: csim.sym_eigen_device_form(b1 + 1, 1)) == ERR_UNSUPPORTED
