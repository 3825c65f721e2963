"""The ensemble-space calls on the GPU (csim_ensemble_gram, _project, _transform, _eofs) against the numpy restatements
of the block in include/csim.h (tests/espace_restatement.py, pinned by tests/test_espace_host.py), bit for bit: the Gram
matrix at the seams of its class loop and in every launch form, projection and transform in the register and the LDS
form, the composition behind eofs(), enqueue-only behaviour, stepping parity, lifetime, and the errors."""
import math

import numpy as np
import pytest

import espace_restatement as ref
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def same_bits(got, want):
    """the same 64-bit patterns; a NaN must meet a NaN, but matches any NaN (the sign and payload of a NaN that an
    operation makes is the hardware's choice), as in tests/test_gpu_ensemble_relax.py"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.int64), want[ok].view(np.int64))


def ensemble(csim, X, bc="dddd"):
    B, ny, nx = X.shape[0], X.shape[1] - 2, X.shape[2] - 2
    ens = csim.Ensemble(B, nx, ny, bc=csim.bc_codes(bc))
    ens.upload_all(X)
    return ens


def ring_mask(ny, nx):
    ring = np.ones((ny + 2, nx + 2), dtype=bool)
    ring[1:-1, 1:-1] = False
    return ring


# ---- Gram ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny,M,truth,centered", ref.GRAM_SMALL)
def test_gram_small_shapes(csim, nx, ny, M, truth, centered):
    B = M + (truth != "none")
    t = ref.truth_of(truth, B)
    X = ref.members(B, nx, ny, seed=1)
    ens = ensemble(csim, X)
    G = ens.gram(truth_member=t, centered=bool(centered))
    ens.close()
    assert G.shape == (M, M)
    assert same_bits(G, ref.gram(X, t, centered))
    assert np.array_equal(G.view(np.int64), G.T.copy().view(np.int64))


_seam_cache = {}


# seams above 64 members where the raw members are compared too: one for each of the two launch forms taken there
# (65 members: two blocks per lane, 129: four), and the ragged last segments after a full one, whose stale rows either
# staging could walk; the others compare the centered matrix only, to stay quick
SEAMS_BOTH = {(64, 257, 65), (64, 65, 129), *ref.GRAM_CARRY_RAGGED}


def seam_case(nx, ny, M):
    """the members of a seam case and its restated Gram matrices (centered, and where asked raw), computed once"""
    key = (nx, ny, M)
    if key not in _seam_cache:
        X = ref.members(M, nx, ny, seed=2).astype(np.float64)
        both = M <= 64 or key in SEAMS_BOTH
        _seam_cache[key] = (X, {c: ref.gram(X, None, c) for c in ((0, 1) if both else (1,))})
    return _seam_cache[key]


@pytest.mark.parametrize("nx,ny,M", ref.GRAM_SEAMS)
def test_gram_class_loop_seams(csim, nx, ny, M):
    X, want = seam_case(nx, ny, M)
    assert ref.gram_plan(M, nx, ny) == csim.ensemble_gram_plan(M, nx, ny)
    ens = ensemble(csim, X)
    got = {c: ens.gram(centered=bool(c)) for c in want}
    ens.close()
    for c in want:
        assert same_bits(got[c], want[c]), c
        assert np.array_equal(got[c].view(np.int64), got[c].T.copy().view(np.int64))


@pytest.mark.parametrize("form", ref.GRAM_FORMS)
@pytest.mark.parametrize("nx,ny,M", [(5, 13, 12), (64, 1025, 3), (64, 257, 65), (64, 65, 129)])
def test_gram_forms_give_the_same_bits(csim, nx, ny, M, form):
    X = ref.members(M, nx, ny, seed=2)
    ens = ensemble(csim, X)
    base = ens.gram()
    ens.set_option("gram_form", form)
    assert ens.get_option("gram_form") == form
    got = ens.gram()
    ens.close()
    assert same_bits(got, base)
    if (nx, ny, M) == (5, 13, 12):
        assert same_bits(got, ref.gram(X, None, 1))


def test_gram_nan_marks_one_row_and_column(csim):
    M, nx, ny = 6, 7, 9
    X = ref.members(M, nx, ny, seed=4)
    X[4, 3, 5] = np.nan
    ens = ensemble(csim, X)
    G = ens.gram(centered=False)
    Gc = ens.gram(centered=True)
    ens.close()
    want = np.zeros((M, M), dtype=bool)
    want[4, :] = want[:, 4] = True
    assert np.array_equal(np.isnan(G), want)
    assert same_bits(G, ref.gram(X, None, 0))
    assert np.isnan(Gc).all()  # the mean of that cell is NaN: every member's perturbation there


def test_gram_after_a_run(csim):
    B, nx, ny = 12, 130, 67
    X = ref.members(B, nx, ny, seed=5)
    ens = ensemble(csim, X, "dnpd")
    ens.set_physics(0.05, 0.1, np.linspace(-0.5, 0.5, B), 0.25)
    ens.run(5)
    G = ens.gram(truth_member=3)
    Y = ens.download_all()
    ens.close()
    assert not np.array_equal(Y, X)
    assert same_bits(G, ref.gram(Y, 3, 1))


def test_gram_within_the_bound_of_the_exact_sum(csim):
    M, nx, ny = 5, 20, 15
    X = ref.members(M, nx, ny, seed=3)
    ens = ensemble(csim, X)
    G = ens.gram()
    ens.close()
    P = ref.interior_rows(ref.perturbations(X, None, 1)[0])
    exact, bound = ref.gram_exact(P), ref.gram_bound(P, nx, ny)
    for a in range(M):
        for b in range(M):
            assert abs(float(ref.Fraction(float(G[a, b])) - exact[a][b])) <= bound[a, b]


# ---- project ---------------------------------------------------------------------------------------------------------

def with_forms(cases):
    """(nx, ny, M, form) for every project_form that selects an instantiation of its own: above 64 members form 0 is
    already the LDS form that form 1 forces"""
    return [(nx, ny, M, form) for nx, ny, M in cases for form in ref.PROJECT_FORMS if form == 0 or M <= 64]


@pytest.mark.parametrize("nx,ny,M,form", with_forms(ref.PROJECT_CASES))
def test_project(csim, nx, ny, M, form):
    """M forecast members: all of an ensemble of M, or M + 1 less a truth member; K = 1, 2 and M"""
    plain, held_out = ref.members(M, nx, ny, seed=6), ref.members(M + 1, nx, ny, seed=7)
    for X, cases in ((plain, ((1, None, True), (M, None, False))),
                     (held_out, ((min(2, M), (M + 1) // 2, True), (M, 0, True), (1, M, False)))):
        ens = ensemble(csim, X)
        ens.set_option("project_form", form)
        for K, t, centered in cases:
            W = ref.weights(M, K, seed=K)
            got = ens.project(W, truth_member=t, centered=centered)
            assert got.shape == (K, ny + 2, nx + 2)
            assert same_bits(got, ref.project(X, W, t, int(centered))), (K, t, centered)
        ens.close()


def test_project_takes_a_vector_and_leaves_the_members_alone(csim):
    X = ref.members(5, 8, 8, seed=7)
    ens = ensemble(csim, X)
    w = np.array([1.0, -2.0, 0.5, 0.0, 3.0])
    got = ens.project(w)
    after = ens.download_all()
    ens.close()
    assert same_bits(got, ref.project(X, w[:, None], None, 1))
    assert same_bits(after, X)


# ---- transform -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny,M,form", with_forms([(7, 9, 3), (5, 13, 12), (130, 67, 12), (257, 3, 48), (8, 8, 64),
                                                     (1, 300, 20), (7, 9, 65), (8, 8, 128), (5, 13, 256)] +
                                                    # every register step full, and the first M of the next one
                                                    [(7, 9, M) for M in (4, 8, 9, 16, 17, 32, 33, 49)]))
def test_transform(csim, nx, ny, M, form):
    B = M + 1
    X = ref.members(B, nx, ny, seed=8)
    W = np.eye(M) + 0.1 * ref.weights(M, M, seed=1)
    wbar = ref.weights(M, 1, seed=2)[:, 0] * 0.1
    ring = ring_mask(ny, nx)
    for t, wb, centered in ((B // 2, wbar, True), (0, None, True), (B - 1, None, False)):
        ens = ensemble(csim, X)
        ens.set_option("project_form", form)
        ens.transform(W, wb, truth_member=t, centered=centered)
        got = ens.download_all()
        ens.close()
        want = ref.transform(X, W, wb, t, int(centered))
        assert same_bits(got, want), (t, centered)
        assert same_bits(got[:, ring], X[:, ring]) and same_bits(got[t], X[t])
        assert not np.array_equal(got[:, 1:-1, 1:-1], X[:, 1:-1, 1:-1])


@pytest.mark.parametrize("M", [6, 70])
def test_transform_selection_copies_members_exactly(csim, M):
    nx, ny = 9, 7
    X = ref.members(M, nx, ny, seed=9)
    pick = np.random.default_rng(M).integers(0, M, M)
    pick[:3] = [2, 2, 0]  # a duplicate and a move
    sel = np.zeros((M, M))
    sel[pick, np.arange(M)] = 1.0
    ens = ensemble(csim, X)
    ens.transform(sel, centered=False)
    got = ens.download_all()
    ens.close()
    np.testing.assert_array_equal(got[:, 1:-1, 1:-1], X[pick][:, 1:-1, 1:-1])
    ring = ring_mask(ny, nx)
    assert same_bits(got[:, ring], X[:, ring])


def test_transform_then_run_matches_upload_then_run(csim):
    B, nx, ny = 8, 40, 33
    X = ref.members(B, nx, ny, seed=10)
    W = np.eye(B - 1) + 0.05 * ref.weights(B - 1, B - 1, seed=3)
    phys = (0.05, 0.1, np.linspace(-0.5, 0.5, B), 0.25)
    a = ensemble(csim, X, "dnpd")
    a.set_physics(*phys)
    a.run(3)
    mid = a.download_all()
    a.transform(W, truth_member=2)
    a.run(4)
    got = a.download_all()
    a.close()
    b = ensemble(csim, ref.transform(mid, W, None, 2, 1), "dnpd")
    b.set_physics(*phys)
    b.run(4)
    want = b.download_all()
    b.close()
    assert same_bits(got, want)


def test_transform_only_enqueues_and_has_copied_its_weights(csim):
    M, nx, ny = 12, 130, 67
    X = ref.members(M, nx, ny, seed=11)
    W = np.eye(M) + 0.1 * ref.weights(M, M, seed=4)
    wbar = 0.1 * ref.weights(M, 1, seed=5)[:, 0]
    W0, wbar0 = W.copy(), wbar.copy()
    ens = ensemble(csim, X)
    ens.transform(W, wbar)
    W[:] = np.nan
    wbar[:] = np.nan
    got = ens.download_all()
    ens.close()
    assert same_bits(got, ref.transform(X, W0, wbar0, None, 1))


# ---- EOFs ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny,B,t", [(7, 9, 6, None), (130, 67, 12, 5), (8, 8, 66, 0)])
def test_eofs_are_the_composition(csim, nx, ny, B, t):
    X = ref.members(B, nx, ny, seed=12)
    M = B - (t is not None)
    K = min(M - 1, 7)
    ens = ensemble(csim, X)
    e = ens.eofs(K, truth_member=t)
    G = ens.gram(truth_member=t)
    lam, pcs, W, null = ref.eofs_weights(G, K, csim.sym_eigen)
    pat = ens.project(W, truth_member=t)
    no_pat = ens.eofs(K, truth_member=t, patterns=False)
    ens.close()
    pat[null] = 0.0
    assert e.n_valid == int((~null).sum()) == K
    assert same_bits(e.lambda_, lam) and same_bits(e.pcs, pcs) and same_bits(e.patterns, pat)
    assert same_bits(e.variance, lam / (M - 1))
    assert no_pat.patterns is None and same_bits(no_pat.pcs, pcs)
    # what they are for: the perturbations are the patterns weighted by the principal components
    if K == M - 1:
        p = ref.perturbations(X, t, 1)[0]
        np.testing.assert_allclose(np.einsum("kr,rji->kji", e.pcs, e.patterns), p, rtol=0, atol=1e-11)


def test_eof_eigenvalues_sum_to_the_trace(csim):
    """sum of lambda_r over all M - 1 modes against trace(G).  The bound: each of the M eigenvalues of the solver is
    within 8 n 2^-52 ||G||_2 of an eigenvalue of G (the allowance tests/test_espace_host.py holds sym_eigen to), the one
    left out is that of the vector of ones, bounded by the error matrix of the computed G (the norm of
    ref.gram_bound) plus the Rayleigh quotient of ones in the computed G; the sums themselves are exact (fsum)."""
    B, nx, ny = 12, 40, 33
    X = ref.members(B, nx, ny, seed=13)
    ens = ensemble(csim, X)
    e = ens.eofs(B - 1, patterns=False)
    G = ens.gram()
    ens.close()
    P = ref.interior_rows(ref.perturbations(X, None, 1)[0])
    ones = np.ones(B)
    tol = (B * 8.0 * B * 2.0 ** -52 * np.linalg.norm(G, 2) + np.linalg.norm(ref.gram_bound(P, nx, ny))
           + abs(ones @ G @ ones) / B)
    assert abs(math.fsum(e.lambda_.tolist()) - math.fsum(np.diag(G).tolist())) <= tol
    assert e.n_valid == B - 1


def test_eofs_of_a_rank_2_ensemble(csim):
    nx, ny, M = 20, 15, 6
    rng = np.random.default_rng(14)
    base = 3.0 + rng.standard_normal((ny + 2, nx + 2))
    modes = rng.standard_normal((2, ny + 2, nx + 2))
    # dyadic coefficients that sum to zero over the members, dyadic fields: the members lie exactly in a plane
    modes, base = np.round(modes * 64) / 64, np.round(base * 64) / 64
    c = np.array([[1.0, -1.0, 0.5, -0.5, 2.0, -2.0], [0.25, 0.75, -1.0, 1.5, -0.5, -1.0]])
    X = base[None] + np.einsum("rk,rji->kji", c, modes)
    ens = ensemble(csim, X)
    e = ens.eofs(5)
    ens.close()
    assert e.n_valid == 2
    assert not e.patterns[2:].any() and not e.pcs[:, 2:].any()
    assert e.patterns[:2].any() and (e.lambda_[:2] > 0).all()


# ---- lifetime and errors ---------------------------------------------------------------------------------------------

def test_two_ensembles_of_different_size_take_turns(csim):
    XA, XB = ref.members(5, 20, 15, seed=15), ref.members(70, 9, 7, seed=16)
    a, b = ensemble(csim, XA), ensemble(csim, XB)
    wantA, wantB = ref.gram(XA, None, 1), ref.gram(XB, None, 1)
    WA, WB = ref.weights(5, 2), ref.weights(70, 3)
    for _ in range(2):
        assert same_bits(a.gram(), wantA)
        assert same_bits(b.gram(), wantB)
        assert same_bits(a.project(WA), ref.project(XA, WA, None, 1))
        assert same_bits(b.project(WB), ref.project(XB, WB, None, 1))
    a.close()
    assert same_bits(b.gram(), wantB)
    b.close()


def test_close_with_a_transform_enqueued(csim):
    M, nx, ny = 64, 130, 67
    ens = ensemble(csim, ref.members(M, nx, ny, seed=17))
    ens.transform(np.eye(M), np.zeros(M))
    ens.close()
    again = ensemble(csim, ref.members(3, 7, 9, seed=1))
    assert same_bits(again.gram(), ref.gram(ref.members(3, 7, 9, seed=1), None, 1))
    again.close()


def test_errors_and_options(csim):
    def code_of(call):
        with pytest.raises(csim.CsimError) as info:
            call()
        return info.value.code

    X = ref.members(5, 7, 9, seed=18)
    ens = ensemble(csim, X)
    L = csim.lib()
    W = np.zeros((5, 5))
    dp = lambda a: a.ctypes.data_as(csim.C.POINTER(csim.C.c_double))  # noqa: E731
    out = np.zeros((6, 11, 9))
    assert L.csim_ensemble_project(ens._h, -1, 1, 6, dp(np.zeros((5, 6))), dp(out)) == ERR_ARG  # K > M
    assert L.csim_ensemble_project(ens._h, -1, 1, 0, dp(W), dp(out)) == ERR_ARG
    assert L.csim_ensemble_transform(ens._h, -1, 0, dp(W), dp(np.zeros(5))) == ERR_ARG  # wbar, not centered
    assert L.csim_ensemble_gram(ens._h, 5, 1, dp(W)) == ERR_ARG
    assert L.csim_ensemble_gram(ens._h, -1, 2, dp(W)) == ERR_ARG
    assert code_of(lambda: ens.eofs(5)) == ERR_ARG  # n_modes > M - 1
    assert code_of(lambda: ens.eofs(4, truth_member=0)) == ERR_ARG
    assert code_of(lambda: ens.eofs(0)) == ERR_ARG
    for key, top in (("gram_form", 3), ("project_form", 1)):
        assert ens.get_option(key) == 0
        assert code_of(lambda: ens.set_option(key, top + 1)) == ERR_ARG
        assert code_of(lambda: ens.set_option(key, -1)) == ERR_ARG
    assert same_bits(ens.download_all(), X)  # no refused call wrote anything
    ens.close()
    big = csim.Ensemble(258, 1, 1)
    assert code_of(lambda: big.gram()) == ERR_UNSUPPORTED
    assert code_of(lambda: big.gram(truth_member=0)) == ERR_UNSUPPORTED
    big.close()
