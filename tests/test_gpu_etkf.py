"""The ETKF on the GPU (csim_ensemble_obs_gram, csim_ensemble_assimilate_etkf) against the numpy restatements of the
block in include/csim.h (tests/etkf_restatement.py, pinned by tests/test_etkf_host.py), bit for bit: the
observation-space Gram matrix, loglik and the count for point and linear networks with every truth position, at the
seams of its class loop and in every launch form; masked observations that are not read; the analysis against the
composition of the public calls, with the mask and the background check, recorded, between runs; the errors and the
lifetime of a network.  Everything is compared through integer views.  Every test here needs the new entry points."""
import numpy as np
import pytest

import espace_restatement as espace
import etkf_restatement as ref
import obsnet_restatement as obsnet
import obsop_restatement as obsop
import screen_restatement as screen
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 1, 4, 5
GRID = (37, 21, 1.0, 1.0, 2.5)   # nx, ny, dx, dy, loc: windows overlap, the plan has several levels
NOBS = 40


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def same_bits(got, want):
    """the same 64-bit patterns, where a NaN matches any NaN (as in tests/test_gpu_espace.py)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.int64), want[ok].view(np.int64))


def exact_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def symmetric(A):
    return np.array_equal(A.view(np.int64), A.T.copy().view(np.int64))


def ensemble(csim, X, grid=GRID, bcs="dddd"):
    nx, ny, dx, dy, _ = grid
    e = csim.Ensemble(X.shape[0], nx, ny, dx, dy, csim.bc_codes(bcs), 0.5)
    e.upload_all(X)
    return e


def truth_of(where, B):
    return {None: None, "first": 0, "middle": B // 2, "last": B - 1}[where]


def members(B, grid, seed):
    nx, ny = grid[0], grid[1]
    rng = np.random.default_rng([seed, B, nx, ny])
    return 3.0 + rng.standard_normal((ny + 2, nx + 2))[None] + 0.5 * rng.standard_normal((B, ny + 2, nx + 2))


def make_network(csim, rng, grid, kind, nobs=NOBS):
    """(i, j, taps or None, r): point observations with two on one cell; bilinear stations between grid points; 3 x 3
    footprints clipped at the sides"""
    nx, ny = grid[0], grid[1]
    r = rng.uniform(0.5, 2.0, nobs)
    if kind == "bilinear":
        x, y = rng.uniform(1, nx, nobs), rng.uniform(1, ny, nobs)
        x[:4], y[:4] = [1.0, nx, 1.25, nx - 0.5], [1.0, ny, ny - 0.25, 1.5]
        i, j, taps = csim.bilinear_taps(nx, ny, x, y)
        return i, j, tuple(taps), r
    i, j = rng.integers(1, nx + 1, nobs).astype(np.int32), rng.integers(1, ny + 1, nobs).astype(np.int32)
    i[:4], j[:4] = [1, nx, 1, nx], [1, ny, ny, 1]
    i[6], j[6] = i[5], j[5]
    if kind == "box":
        i, j, taps = csim.box_taps(nx, ny, i, j, 1, 1)
        return i, j, tuple(taps), r
    return i, j, None, r


def operator(X, t, i, j, taps):
    """h_k of the forecast members, (M, nobs), input order"""
    if taps is None:
        return X[obsnet.forecast(X.shape[0], t)][:, j, i]
    return obsop.h_members(X, t, i, j, taps)


def order_of(csim, net, i, j):
    info = net.info
    return ref.plan_order(csim.ensemble_assim_plan(i, j, info.lx, info.ly))


def distinct_cells(rng, nx, ny, nobs):
    e = rng.permutation(nx * ny)[:nobs]
    return (e % nx + 1).astype(np.int32), (e // nx + 1).astype(np.int32)


# ---- 1. the matrix: bits ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", [None, "first", "middle", "last"])
@pytest.mark.parametrize("kind", ["point", "bilinear", "box"])
def test_obs_gram_is_the_restatement(csim, kind, where):
    M = 7
    B = M if where is None else M + 1
    t = truth_of(where, B)
    rng = np.random.default_rng([1, B, len(kind)])
    X = members(B, GRID, 1)
    i, j, taps, r = make_network(csim, rng, GRID, kind)
    y = 3.0 + rng.standard_normal(NOBS)
    mask = np.ones(NOBS, dtype=np.uint8)
    mask[[2, 11, 39]] = 0
    e = ensemble(csim, X)
    net = e.obs_network(i, j, r, GRID[4], taps=taps)
    net.set_values(y)
    order = order_of(csim, net, i, j)
    assert net.info.nlevels > 1 and not np.array_equal(order, np.arange(NOBS))
    H = operator(X, t, i, j, taps)
    full = e.obs_gram(net, truth_member=t, loglik=True)
    net.set_active(mask)
    part = e.obs_gram(net, truth_member=t, loglik=True)
    bare = e.obs_gram(net, truth_member=t)
    assert exact_bits(e.download_all(), X)
    e.close()
    for got, used in ((full, np.ones(NOBS, dtype=bool)), (part, mask == 1)):
        A, ll, n = ref.obs_gram(H, y, r, used, order, loglik=True)
        assert got.A.shape == (M + 1, M + 1) and got.loglik.shape == (M,)
        assert same_bits(got.A, A) and same_bits(got.loglik, ll) and got.n_used == n
        assert symmetric(got.A)
    assert bare.loglik is None and exact_bits(bare.A, part.A) and bare.n_used == NOBS - 3


_cache = {}


def seam_case(csim, nx, ny, M, nobs):
    """members, distinct observed cells, values and the restated results of a seam case, computed once.  loc < dx / 2:
    lx = ly = 0, distinct cells never conflict, the plan is one level in input order"""
    key = (nx, ny, M, nobs)
    if key not in _cache:
        rng = np.random.default_rng([2, nx, ny, M, nobs])
        X = members(M, (nx, ny), 2)
        i, j = distinct_cells(rng, nx, ny, nobs)
        r = rng.uniform(0.5, 2.0, nobs)
        y = 3.0 + rng.standard_normal(nobs)
        want = ref.obs_gram(X[:, j, i], y, r, True, np.arange(nobs), loglik=True)
        _cache[key] = (X, i, j, r, y, want)
    return _cache[key]


def run_seam(csim, nx, ny, M, nobs, forms=(0,)):
    X, i, j, r, y, want = seam_case(csim, nx, ny, M, nobs)
    assert csim.obs_gram_plan(M, nobs) == ref.gram_plan(M, nobs)
    e = ensemble(csim, X, (nx, ny, 1.0, 1.0, 0.4))
    net = e.obs_network(i, j, r, 0.4)
    assert (net.info.lx, net.info.ly, net.info.nlevels) == (0, 0, 1)
    net.set_values(y)
    for form in forms:
        e.set_option("obs_gram_form", form)
        assert e.get_option("obs_gram_form") == form
        got = e.obs_gram(net, loglik=True)
        assert same_bits(got.A, want[0]) and same_bits(got.loglik, want[1]) and got.n_used == want[2] == nobs, form
        assert symmetric(got.A)
    e.close()


@pytest.mark.parametrize("nobs", [1, 63, 64, 65])
def test_obs_gram_segment_seams(csim, nobs):
    run_seam(csim, 16, 16, 8, nobs)


# nseg = cap and cap + 1 for each cap of the class loop
@pytest.mark.parametrize("nx,ny,M,nobs", [(256, 257, 8, 65536), (256, 257, 8, 65537), (128, 129, 65, 16385),
                                          (64, 65, 129, 4097)])
def test_obs_gram_class_loop_seams(csim, nx, ny, M, nobs):
    nseg, Gc = ref.gram_plan(M, nobs)
    assert nseg in (Gc, Gc + 1) and Gc in (1024, 256, 64)
    run_seam(csim, nx, ny, M, nobs)


@pytest.mark.parametrize("M", [2, 63, 64, 65, 255, 256])
def test_obs_gram_member_seams(csim, M):
    run_seam(csim, 16, 16, M, 100)


@pytest.mark.parametrize("M,nobs", [(12, 100), (65, 200), (129, 100)])
def test_obs_gram_forms_give_the_same_bits(csim, M, nobs):
    run_seam(csim, 16, 16, M, nobs, forms=(1, 2, 3, 0))


def test_obs_gram_forms_on_a_linear_network(csim):
    M = 12
    rng = np.random.default_rng(31)
    X = members(M, GRID, 31)
    i, j, taps, r = make_network(csim, rng, GRID, "box")
    y = 3.0 + rng.standard_normal(NOBS)
    e = ensemble(csim, X)
    net = e.obs_network(i, j, r, GRID[4], taps=taps)
    net.set_values(y)
    want = ref.obs_gram(operator(X, None, i, j, taps), y, r, True, order_of(csim, net, i, j), loglik=True)
    for form in (0, 1, 2, 3):
        e.set_option("obs_gram_form", form)
        got = e.obs_gram(net, loglik=True)
        assert same_bits(got.A, want[0]) and same_bits(got.loglik, want[1]), form
    with pytest.raises(csim.CsimError) as ei:
        e.set_option("obs_gram_form", 4)
    assert ei.value.code == ERR_ARG
    e.close()


# ---- 2. masked observations are not read -------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["point", "box"])
def test_masked_observations_are_not_read(csim, kind):
    M, t = 6, 2
    rng = np.random.default_rng([41, len(kind)])
    X = members(M + 1, GRID, 41)
    i, j, taps, r = make_network(csim, rng, GRID, kind)
    # observation 9 on a cell of its own, far from every other footprint
    i[9], j[9] = 20, 11
    keep = (np.abs(i - 20) > 2) | (np.abs(j - 11) > 2)
    keep[9] = True
    i, j, r = i[keep], j[keep], r[keep]
    nobs = len(i)
    o = int(np.flatnonzero((i == 20) & (j == 11))[0])
    if kind == "box":
        i, j, taps = csim.box_taps(GRID[0], GRID[1], i, j, 1, 1)
        taps = tuple(taps)
    y = 3.0 + rng.standard_normal(nobs)
    X[4, 11, 20] = np.nan
    mask = np.ones(nobs, dtype=np.uint8)
    mask[o] = 0
    e = ensemble(csim, X)
    net = e.obs_network(i, j, r, GRID[4], taps=taps)
    net.set_values(y)
    net.set_active(mask)
    order = order_of(csim, net, i, j)
    got = e.obs_gram(net, truth_member=t, loglik=True)
    H = operator(X, t, i, j, taps)
    assert np.isnan(H[:, o]).any() and not np.isnan(np.delete(H, o, axis=1)).any()
    want = ref.obs_gram(H, y, r, mask == 1, order, loglik=True)
    assert np.isfinite(got.A).all() and np.isfinite(got.loglik).all() and got.n_used == nobs - 1
    assert exact_bits(got.A, want[0]) and exact_bits(got.loglik, want[1])
    res = e.assimilate_etkf(net, truth_member=t)
    assert res.n_used == nobs - 1 and np.isfinite(res.chi2)
    # the same observation used: A is NaN, and the analysis refuses and leaves the members alone
    e.upload_all(X)
    net.set_active(None)
    bad = e.obs_gram(net, truth_member=t, loglik=True)
    assert np.isnan(bad.A).any() and same_bits(bad.A, ref.obs_gram(H, y, r, True, order)[0])
    with pytest.raises(csim.CsimError) as ei:
        e.assimilate_etkf(net, truth_member=t)
    assert ei.value.code == ERR_STATE
    assert exact_bits(e.download_all(), X)
    e.close()


# ---- 3. the analysis ---------------------------------------------------------------------------------------------------

def ring_of(grid):
    ring = np.ones((grid[1] + 2, grid[0] + 2), dtype=bool)
    ring[1:-1, 1:-1] = False
    return ring


ANALYSES = [("point", 5, None, 1.0), ("point", 8, "first", 1.1), ("bilinear", 12, "middle", 1.1),
            ("box", 33, "last", 1.0), ("point", 65, None, 1.1)]


@pytest.mark.parametrize("case", ANALYSES, ids=[f"{c[0]}_M{c[1]}_t{c[2]}_lam{c[3]}" for c in ANALYSES])
def test_analysis_is_the_composition_of_the_public_calls(csim, case):
    kind, M, where, lam = case
    B = M if where is None else M + 1
    t = truth_of(where, B)
    rng = np.random.default_rng([51, M])
    X = members(B, GRID, 51)
    i, j, taps, r = make_network(csim, rng, GRID, kind)
    y = 3.0 + rng.standard_normal(NOBS)
    mask = np.ones(NOBS, dtype=np.uint8)
    mask[[1, 30]] = 0
    a, b = ensemble(csim, X, bcs="dnpd"), ensemble(csim, X, bcs="dnpd")
    na, nb = (e.obs_network(i, j, r, GRID[4], taps=taps) for e in (a, b))
    for n in (na, nb):
        n.set_values(y)
        n.set_active(mask)
    res = a.assimilate_etkf(na, inflation=lam, truth_member=t)
    g = b.obs_gram(nb, truth_member=t)
    w = csim.etkf_weights(g.A, lam)
    b.transform(w.W, w.wbar, truth_member=t)
    A, Bc = a.download_all(), b.download_all()
    assert exact_bits(A, Bc) and not exact_bits(A, X)
    assert res.n_used == g.n_used == NOBS - 2 and exact_bits(res.chi2, g.A[M, M])
    assert exact_bits(res.gamma, w.gamma) and exact_bits(res.dfs, w.dfs)
    assert np.array_equal(na.status(), np.where(mask == 1, screen.USED, screen.INACTIVE))
    # and the whole chain is the restatement's
    A0 = ref.obs_gram(operator(X, t, i, j, taps), y, r, mask == 1, order_of(csim, na, i, j))[0]
    W, wbar, gamma, dfs, _ = ref.etkf_weights(A0, lam, csim.sym_eigen)
    assert exact_bits(g.A, A0) and exact_bits(w.W, W) and exact_bits(w.wbar, wbar)
    assert same_bits(A, espace.transform(X, W, wbar, t, True))
    # the ghost ring and the truth member keep their bits
    assert exact_bits(A[:, ring_of(GRID)], X[:, ring_of(GRID)])
    if t is not None:
        assert exact_bits(A[t], X[t])
    a.close(), b.close()


def test_background_check_is_the_composition_with_those_observations_masked(csim):
    M, t, tol, lam = 9, 3, 3.0, 1.05
    rng = np.random.default_rng(61)
    X = members(M + 1, GRID, 61)
    i, j, taps, r = make_network(csim, rng, GRID, "bilinear")
    hb, vb = obsop.mv(X, t, i, j, taps)
    y = hb + 0.5 * np.sqrt(vb + r) * rng.standard_normal(NOBS).clip(-2, 2)
    y[8] = hb[8] + 50.0 * np.sqrt(vb[8] + r[8])     # a gross error
    y[21] = hb[21] - 40.0 * np.sqrt(vb[21] + r[21])
    mask = np.ones(NOBS, dtype=np.uint8)
    mask[[3, 12]] = 0
    st = np.array([csim.obs_screen_decide(y[o], hb[o], vb[o], r[o], tol, int(mask[o])) for o in range(NOBS)],
                  dtype=np.uint8)
    assert st[8] == st[21] == screen.REJECTED and set(st.tolist()) == {0, 1, 2}
    a, b = ensemble(csim, X), ensemble(csim, X)
    na, nb = (e.obs_network(i, j, r, GRID[4], taps=taps) for e in (a, b))
    na.set_values(y), nb.set_values(y)
    na.set_active(mask)
    nb.set_active(st == screen.USED)
    res = a.assimilate_etkf(na, inflation=lam, truth_member=t, screen=tol)
    assert np.array_equal(na.status(), st) and res.n_used == np.count_nonzero(st == 0)
    g = b.obs_gram(nb, truth_member=t)
    w = csim.etkf_weights(g.A, lam)
    b.transform(w.W, w.wbar, truth_member=t)
    assert exact_bits(res.chi2, g.A[M, M]) and exact_bits(res.gamma, w.gamma)
    assert exact_bits(a.download_all(), b.download_all())
    a.close(), b.close()


@pytest.mark.parametrize("lam", [1.0, 1.1])
def test_all_masked(csim, lam):
    """with inflation 1 nothing is launched and the members keep their bits; with inflation the spread alone grows"""
    M = 6
    rng = np.random.default_rng(71)
    X = members(M, GRID, 71)
    i, j, _, r = make_network(csim, rng, GRID, "point")
    e = ensemble(csim, X)
    net = e.obs_network(i, j, r, GRID[4])
    net.set_values(rng.standard_normal(NOBS))
    net.set_active(np.zeros(NOBS, dtype=np.uint8))
    res = e.assimilate_etkf(net, inflation=lam)
    A = e.download_all()
    assert res.n_used == 0 and res.chi2 == 0.0 and res.dfs == 0.0 and not res.gamma.any()
    assert (net.status() == screen.INACTIVE).all()
    if lam == 1.0:
        assert exact_bits(A, X)
    else:
        W, wbar = csim.etkf_weights(np.zeros((M + 1, M + 1)), lam)[:2]
        assert same_bits(A, espace.transform(X, W, wbar, None, True)) and not exact_bits(A, X)
        np.testing.assert_allclose(A[:, 1:-1, 1:-1].std(axis=0), lam * X[:, 1:-1, 1:-1].std(axis=0), rtol=1e-12)
    e.close()


def test_recorded_analysis_fills_fetch_and_both_logs(csim):
    M, t, tol = 9, 0, 4.0
    rng = np.random.default_rng(81)
    X = members(M + 1, GRID, 81)
    i, j, _, r = make_network(csim, rng, GRID, "point")
    hb, vb = obsnet.mv(X, t, i, j)
    y = hb + 0.5 * np.sqrt(vb + r) * rng.standard_normal(NOBS).clip(-2, 2)
    y[8] = hb[8] + 50.0 * np.sqrt(vb[8] + r[8])
    mask = np.ones(NOBS, dtype=np.uint8)
    mask[[3, 12, 20]] = 0
    st = screen.statuses(y, hb, vb, r, tol, mask)
    assert st[8] == screen.REJECTED
    a, b = ensemble(csim, X), ensemble(csim, X)
    na, nb = (e.obs_network(i, j, r, GRID[4], log_cycles=2) for e in (a, b))
    for n in (na, nb):
        n.set_values(y)
        n.set_active(mask)
    a.assimilate_etkf(na, truth_member=t, record=True, screen=tol)
    b.assimilate_network(nb, truth_member=t, record=True, screen=tol)   # the serial analysis of a copy
    A = a.download_all()
    fa, fb = na.fetch(), nb.fetch()
    assert exact_bits(fa.bg_mean, fb.bg_mean) and exact_bits(fa.bg_var, fb.bg_var)
    assert same_bits(fa.bg_mean, hb) and same_bits(fa.bg_var, vb) and exact_bits(fa.y, y)
    ha, va = obsnet.mv(A, t, i, j)
    assert same_bits(fa.post_mean, ha) and same_bits(fa.post_var, va)
    assert np.array_equal(na.status(), st) and np.array_equal(nb.status(), st)
    log, slog = na.log(), na.screen_log()
    assert len(log) == 1 and len(slog) == 1
    rec, srec = screen.cycle(y, hb, vb, ha, va, r, st), screen.screen_cycle(st)
    assert all(exact_bits(log[0][k], rec[k]) for k in obsnet.FIELDS), (log[0], rec)
    assert all(exact_bits(slog[0][k], srec[k]) for k in screen.SCREEN_FIELDS), (slog[0], srec)
    # the analysis pulls the mean towards the observations it used
    used = st == screen.USED
    assert np.sum((y - ha)[used] ** 2 / r[used]) < np.sum((y - hb)[used] ** 2 / r[used])
    # a second record goes on; a third finds the log full and changes nothing
    a.assimilate_etkf(na, truth_member=t, record=True)
    assert len(na.log()) == 2 and na.screen_log()[1]["n_inactive"] == 3.0
    before = a.download_all()
    with pytest.raises(csim.CsimError) as ei:
        a.assimilate_etkf(na, truth_member=t, record=True)
    assert ei.value.code == ERR_STATE and exact_bits(a.download_all(), before)
    a.close(), b.close()


def test_run_analysis_run_is_upload_of_the_result_and_run(csim):
    B, t = 8, 5
    rng = np.random.default_rng(91)
    X = members(B, GRID, 91)
    i, j, taps, r = make_network(csim, rng, GRID, "bilinear")
    phys = (0.05, 0.1, list(np.linspace(-0.5, 0.5, B)), 0.25)
    a, b = ensemble(csim, X, bcs="dnpd"), ensemble(csim, X, bcs="dnpd")
    a.set_physics(*phys), b.set_physics(*phys)
    net = a.obs_network(i, j, r, GRID[4], taps=taps)
    a.run(5)
    net.observe(t, seed=7)
    a.assimilate_etkf(net, inflation=1.05, truth_member=t)
    mid = a.download_all()
    a.run(6)
    b.upload_all(mid)
    b.run(6)
    assert exact_bits(a.download_all(), b.download_all())
    a.close(), b.close()


# ---- 4. errors and lifetime ------------------------------------------------------------------------------------------

def code_of(csim, call):
    with pytest.raises(csim.CsimError) as info:
        call()
    return info.value.code


def test_errors(csim):
    rng = np.random.default_rng(95)
    grid = (8, 8, 1.0, 1.0, 2.5)
    X = members(4, grid, 95)
    i, j, r = np.array([2, 5], dtype=np.int32), np.array([3, 6], dtype=np.int32), np.array([1.0, 0.5])
    e, other = ensemble(csim, X, grid), ensemble(csim, X, grid)
    net = e.obs_network(i, j, r, 2.5, log_cycles=1)
    for call in (lambda **k: e.obs_gram(net, **k), lambda **k: e.assimilate_etkf(net, **k)):
        assert code_of(csim, call) == ERR_STATE                                # no values yet
    net.set_values(rng.standard_normal(2))
    for call in (lambda: other.obs_gram(net), lambda: other.assimilate_etkf(net)):
        assert code_of(csim, call) == ERR_ARG                                  # another ensemble's network
    for call in (lambda **k: e.obs_gram(net, **k), lambda **k: e.assimilate_etkf(net, **k)):
        assert code_of(csim, lambda: call(truth_member=4)) == ERR_ARG
        assert code_of(csim, lambda: call(truth_member=-2)) == ERR_ARG
    for bad in (0.99, -1.0, np.nan, np.inf):
        assert code_of(csim, lambda: e.assimilate_etkf(net, inflation=bad)) == ERR_ARG
    assert code_of(csim, lambda: e.assimilate_etkf(net, screen=-1.0)) == ERR_ARG
    assert code_of(csim, lambda: e.assimilate_etkf(net, record=2)) == ERR_ARG
    assert exact_bits(e.download_all(), X)
    e.assimilate_etkf(net, record=True)
    after = e.download_all()
    assert code_of(csim, lambda: e.assimilate_etkf(net, record=True)) == ERR_STATE   # the log is full
    assert exact_bits(e.download_all(), after)
    # M = 1 and M = 257
    two = ensemble(csim, X[:2], grid)
    n2 = two.obs_network(i, j, r, 2.5)
    n2.set_values(np.zeros(2))
    for call in (lambda: two.obs_gram(n2, truth_member=0), lambda: two.assimilate_etkf(n2, truth_member=1)):
        assert code_of(csim, call) == ERR_ARG
    assert two.obs_gram(n2).A.shape == (3, 3)
    big = csim.Ensemble(258, 4, 4, 1.0, 1.0, csim.bc_codes("dddd"), 0.5)
    nb = big.obs_network([2], [2], [1.0], 2.5)
    nb.set_values(np.zeros(1))
    for call in (lambda: big.obs_gram(nb), lambda: big.assimilate_etkf(nb), lambda: big.obs_gram(nb, truth_member=0),
                 lambda: big.assimilate_etkf(nb, truth_member=257)):
        assert code_of(csim, call) == ERR_UNSUPPORTED
    L = csim.lib()
    assert L.csim_ensemble_obs_gram(None, None, -1, None, None, None) == ERR_ARG
    assert L.csim_ensemble_assimilate_etkf(None, None, 1.0, -1, 0, 0.0) == ERR_ARG
    assert L.csim_ensemble_etkf_info(None, None, None, None, None, None) == ERR_ARG
    assert L.csim_ensemble_etkf_info(other._h, None, None, None, None, None) == ERR_STATE   # no analysis yet
    for x in (e, other, two, big):
        x.close()


def test_a_network_destroyed_by_its_ensemble(csim):
    X = members(4, (8, 8), 97)
    grid = (8, 8, 1.0, 1.0, 2.5)
    e, other = ensemble(csim, X, grid), ensemble(csim, X, grid)
    net = e.obs_network([2, 5], [3, 6], [1.0, 0.5], 2.5)
    net.set_values(np.zeros(2))
    assert e.obs_gram(net).n_used == 2
    e.assimilate_etkf(net)
    e.close()                       # destroys the network; its Python handle is cleared
    assert net._h is None
    assert code_of(csim, lambda: other.obs_gram(net)) == ERR_ARG
    assert code_of(csim, lambda: other.assimilate_etkf(net)) == ERR_ARG
    net.close()
    other.close()
