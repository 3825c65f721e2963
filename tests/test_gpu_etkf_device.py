"""The ETKF that only enqueues (csim_ensemble_assimilate_etkf_device) against the composition of the public calls on a
copy of the ensemble, obs_gram -> etkf_weights(order = round robin) -> transform, bit for bit, ghost ring and truth member
included: every member count at which the eigensolver or the transform changes its form, bilinear and box networks,
masked and rejected observations, recorded cycles, the skip and the non-finite status, three cycles without a fetch, the
info, and the unchanged host path.  Everything is compared through integer views.  Every test here needs the new entry
points."""
import numpy as np
import pytest

import obsnet_restatement as obsnet
import obsop_restatement as obsop
import screen_restatement as screen
from __graft_entry__ import load_package
from test_gpu_etkf import ensemble, exact_bits, make_network, members, ring_of, same_bits, truth_of

pytestmark = pytest.mark.gpu

ERR_STATE, ERR_UNSUPPORTED = 4, 5
GRID = (24, 20, 1.0, 1.0, 2.5)
SMALL = (8, 8, 1.0, 1.0, 2.5)
NOBS = 100


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def compose(csim, b, nb, lam, t):
    """the host composition on the copy; returns (g, w)"""
    g = b.obs_gram(nb, truth_member=t)
    w = csim.etkf_weights(g.A, lam, order="round_robin")
    if g.n_used != 0 or lam != 1.0:
        b.transform(w.W, w.wbar, truth_member=t)
    return g, w


def info_is(info, g, w, M):
    return (info.n_used == g.n_used and exact_bits(info.chi2, g.A[M, M]) and exact_bits(info.gamma, w.gamma)
            and exact_bits(info.dfs, w.dfs) and info.sweeps == w.sweeps and info.status == 0)


CASES = [("bilinear", 2, None, 1.0, GRID), ("box", 5, "first", 1.1, GRID), ("bilinear", 63, "middle", 1.1, GRID),
         ("box", 64, "last", 1.0, GRID), ("bilinear", 65, None, 1.05, GRID), ("box", 129, "first", 1.1, GRID),
         ("bilinear", 256, None, 1.1, SMALL)]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}_M{c[1]}_t{c[2]}_lam{c[3]}" for c in CASES])
def test_device_analysis_is_the_composition_in_the_round_robin_order(csim, case):
    kind, M, where, lam, grid = case
    B = M if where is None else M + 1
    t = truth_of(where, B)
    rng = np.random.default_rng([52, M])
    X = members(B, grid, 52)
    i, j, taps, r = make_network(csim, rng, grid, kind, NOBS)
    y = 3.0 + rng.standard_normal(NOBS)
    mask = np.ones(NOBS, dtype=np.uint8)
    mask[[1, 30, 99]] = 0
    a, b = ensemble(csim, X, grid, bcs="dnpd"), ensemble(csim, X, grid, bcs="dnpd")
    na, nb = (e.obs_network(i, j, r, grid[4], taps=taps) for e in (a, b))
    for n in (na, nb):
        n.set_values(y)
        n.set_active(mask)
    assert a.assimilate_etkf(na, inflation=lam, truth_member=t, device=True) is None
    g, w = compose(csim, b, nb, lam, t)
    A, Bc = a.download_all(), b.download_all()
    assert exact_bits(A, Bc) and not exact_bits(A, X)
    assert info_is(a.etkf_info(), g, w, M) and g.n_used == NOBS - 3
    assert np.array_equal(na.status(), np.where(mask == 1, screen.USED, screen.INACTIVE))
    assert exact_bits(A[:, ring_of(grid)], X[:, ring_of(grid)])
    if t is not None:
        assert exact_bits(A[t], X[t])
    a.close(), b.close()


@pytest.mark.parametrize("form", [1, 2, 3])
def test_every_eigen_form_gives_the_same_members(csim, form):
    M, lam = 12, 1.1
    rng = np.random.default_rng(53)
    X = members(M, GRID, 53)
    i, j, taps, r = make_network(csim, rng, GRID, "bilinear", NOBS)
    y = 3.0 + rng.standard_normal(NOBS)
    a, b = ensemble(csim, X, GRID), ensemble(csim, X, GRID)
    na, nb = (e.obs_network(i, j, r, GRID[4], taps=taps) for e in (a, b))
    na.set_values(y), nb.set_values(y)
    a.set_option("eigen_form", form)
    assert a.get_option("eigen_form") == form
    a.assimilate_etkf(na, inflation=lam, device=True)
    g, w = compose(csim, b, nb, lam, None)
    assert exact_bits(a.download_all(), b.download_all()) and info_is(a.etkf_info(), g, w, M)
    with pytest.raises(csim.CsimError):
        a.set_option("eigen_form", 4)
    a.close(), b.close()


def test_a_forced_form_that_does_not_admit_the_members_is_unsupported(csim):
    M = csim.sym_eigen_device_form(1, 1)[1] + 1
    rng = np.random.default_rng(54)
    X = members(M, SMALL, 54)
    i, j, _, r = make_network(csim, rng, SMALL, "point", 10)
    e = ensemble(csim, X, SMALL)
    net = e.obs_network(i, j, r, SMALL[4])
    net.set_values(rng.standard_normal(10))
    e.set_option("eigen_form", 1)
    with pytest.raises(csim.CsimError) as ei:
        e.assimilate_etkf(net, device=True)
    assert ei.value.code == ERR_UNSUPPORTED and exact_bits(e.download_all(), X)
    e.close()


def test_background_check_and_record(csim):
    M, t, tol, lam = 9, 3, 3.0, 1.05
    rng = np.random.default_rng(61)
    X = members(M + 1, GRID, 61)
    i, j, taps, r = make_network(csim, rng, GRID, "bilinear", NOBS)
    hb, vb = obsop.mv(X, t, i, j, taps)
    y = hb + 0.5 * np.sqrt(vb + r) * rng.standard_normal(NOBS).clip(-2, 2)
    y[8] = hb[8] + 50.0 * np.sqrt(vb[8] + r[8])     # gross errors
    y[21] = hb[21] - 40.0 * np.sqrt(vb[21] + r[21])
    mask = np.ones(NOBS, dtype=np.uint8)
    mask[[3, 12]] = 0
    st = screen.statuses(y, hb, vb, r, tol, mask)
    assert st[8] == st[21] == screen.REJECTED and set(st.tolist()) == {0, 1, 2}
    a, b, c = (ensemble(csim, X, GRID) for _ in range(3))
    na, nb, nc = (e.obs_network(i, j, r, GRID[4], taps=taps, log_cycles=2) for e in (a, b, c))
    for n in (na, nb, nc):
        n.set_values(y)
    na.set_active(mask), nc.set_active(mask)
    nb.set_active(st == screen.USED)
    a.assimilate_etkf(na, inflation=lam, truth_member=t, screen=tol, record=True, device=True)
    g, w = compose(csim, b, nb, lam, t)
    c.assimilate_etkf(nc, inflation=lam, truth_member=t, screen=tol, record=True)   # the host path
    A = a.download_all()
    assert exact_bits(A, b.download_all())
    assert np.array_equal(na.status(), st) and info_is(a.etkf_info(), g, w, M)
    assert g.n_used == np.count_nonzero(st == screen.USED)
    # what is taken before the transform is the host path's, bit for bit; the rest is the restatement's on these members
    fa, fc = na.fetch(), nc.fetch()
    assert exact_bits(fa.bg_mean, fc.bg_mean) and exact_bits(fa.bg_var, fc.bg_var) and exact_bits(fa.y, fc.y)
    ha, va = obsop.mv(A, t, i, j, taps)
    assert same_bits(fa.post_mean, ha) and same_bits(fa.post_var, va)
    np.testing.assert_allclose(fa.post_mean, fc.post_mean, rtol=0, atol=1e-11)
    log, slog = na.log(), na.screen_log()
    assert len(log) == 1 and len(slog) == 1
    rec = screen.cycle(y, hb, vb, ha, va, r, st)
    assert all(exact_bits(log[0][k], rec[k]) for k in obsnet.FIELDS), (log[0], rec)
    assert all(exact_bits(slog[0][k], nc.screen_log()[0][k]) for k in screen.SCREEN_FIELDS)
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("lam", [1.0, 1.05])
def test_all_masked_skips_or_only_inflates(csim, lam):
    M = 6
    rng = np.random.default_rng(71)
    X = members(M, GRID, 71)
    i, j, _, r = make_network(csim, rng, GRID, "point", NOBS)
    a, b = ensemble(csim, X, GRID), ensemble(csim, X, GRID)
    na, nb = (e.obs_network(i, j, r, GRID[4]) for e in (a, b))
    for n in (na, nb):
        n.set_values(rng.standard_normal(NOBS))
        n.set_active(np.zeros(NOBS, dtype=np.uint8))
    a.assimilate_etkf(na, inflation=lam, device=True)
    g, w = compose(csim, b, nb, lam, None)
    A = a.download_all()
    info = a.etkf_info()
    assert info.n_used == 0 and info.chi2 == 0.0 and info.dfs == 0.0 and not info.gamma.any() and info.sweeps == 0
    assert exact_bits(A, b.download_all())
    assert exact_bits(A, X) if lam == 1.0 else not exact_bits(A, X)
    a.close(), b.close()


def test_a_non_finite_gram_matrix_leaves_the_members_and_fails_the_info(csim):
    M = 7
    rng = np.random.default_rng(72)
    X = members(M, GRID, 72)
    i, j, _, r = make_network(csim, rng, GRID, "point", NOBS)
    y = 3.0 + rng.standard_normal(NOBS)
    bad = X.copy()
    bad[2, j[10], i[10]] = np.nan   # under a used observation
    a, b = ensemble(csim, bad, GRID), ensemble(csim, X, GRID)
    na, nb = (e.obs_network(i, j, r, GRID[4]) for e in (a, b))
    na.set_values(y), nb.set_values(y)
    a.assimilate_etkf(na, inflation=1.1, device=True)
    assert same_bits(a.download_all(), bad)
    for _ in range(2):
        with pytest.raises(csim.CsimError) as ei:
            a.etkf_info()
        assert ei.value.code == ERR_STATE
    # a clean analysis on the same handle works
    a.upload_all(X)
    a.assimilate_etkf(na, inflation=1.1, device=True)
    g, w = compose(csim, b, nb, 1.1, None)
    assert exact_bits(a.download_all(), b.download_all()) and info_is(a.etkf_info(), g, w, M)
    a.close(), b.close()


def test_three_cycles_without_a_fetch(csim):
    B, t, lam = 8, 5, 1.05
    rng = np.random.default_rng(91)
    X = members(B, GRID, 91)
    i, j, taps, r = make_network(csim, rng, GRID, "bilinear", NOBS)
    phys = (0.05, 0.1, list(np.linspace(-0.5, 0.5, B)), 0.25)
    a, b = ensemble(csim, X, GRID, bcs="dnpd"), ensemble(csim, X, GRID, bcs="dnpd")
    a.set_physics(*phys), b.set_physics(*phys)
    na, nb = (e.obs_network(i, j, r, GRID[4], taps=taps) for e in (a, b))
    for cycle in range(3):
        a.run(4)
        na.observe(t, seed=7 + cycle)
        a.assimilate_etkf(na, inflation=lam, truth_member=t, device=True)
        a.perturb(0.01, 3.0, seed=11, draw=cycle, truth_member=t)
    last = None
    for cycle in range(3):
        b.run(4)
        nb.observe(t, seed=7 + cycle)
        last = compose(csim, b, nb, lam, t)
        b.perturb(0.01, 3.0, seed=11, draw=cycle, truth_member=t)
    assert exact_bits(a.download_all(), b.download_all())
    assert info_is(a.etkf_info(), *last, B - 1)
    a.close(), b.close()


def test_the_host_path_keeps_its_bits_and_its_info(csim):
    M, lam = 9, 1.1
    rng = np.random.default_rng(95)
    X = members(M, GRID, 95)
    i, j, _, r = make_network(csim, rng, GRID, "point", NOBS)
    y = 3.0 + rng.standard_normal(NOBS)
    a, b = ensemble(csim, X, GRID), ensemble(csim, X, GRID)
    na, nb = (e.obs_network(i, j, r, GRID[4]) for e in (a, b))
    na.set_values(y), nb.set_values(y)
    a.assimilate_etkf(na, inflation=lam, device=True)   # a device analysis before it leaves nothing behind
    a.upload_all(X)
    res = a.assimilate_etkf(na, inflation=lam)
    g = b.obs_gram(nb)
    w = csim.etkf_weights(g.A, lam)
    b.transform(w.W, w.wbar)
    assert exact_bits(a.download_all(), b.download_all())
    assert exact_bits(res.gamma, w.gamma) and exact_bits(res.dfs, w.dfs) and res.n_used == NOBS
    info = a.etkf_info()
    assert exact_bits(info.gamma, w.gamma) and info.sweeps == 0 and info.status == 0
    rr = csim.etkf_weights(g.A, lam, order="round_robin")
    assert not exact_bits(rr.W, w.W)   # the two orders differ in the last bits: the comparison above tells them apart
    a.close(), b.close()
