"""The 4D-ETKF on the GPU (csim_obs_network_set_slots, _hold, _observe_slot, _held, csim_ensemble_obs_gram_held,
csim_ensemble_assimilate_etkf_held) against the numpy restatements (tests/held_restatement.py, pinned by
tests/test_held_host.py, on top of the ETKF's), bit for bit: the held rows of point and linear networks, slot by slot;
the Gram matrix from rows against the one from the state, at the segment seams and in every launch form; several slots
held from different states; the held analysis against the composition of the public calls on both paths, its screening
and its record from the rows; observe by slot; the errors and the state rules; and the claim itself, a hold, a run and
a held analysis against an analysis and the same run, within a tolerance measured on the CPU.  Everything but that last
test is compared through integer views.  Every test here needs the new entry points."""
import numpy as np
import pytest

import espace_restatement as espace
import etkf_restatement as ref
import held_restatement as held
import obsnet_restatement as obsnet
import obsop_restatement as obsop
import screen_restatement as screen
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 1, 4, 5
GRID = (37, 21, 1.0, 1.0, 2.5)   # nx, ny, dx, dy, loc: windows overlap, the plan has several levels
NOBS = 40

# the reference's own disagreement between the two paths of test_hold_run_analysis_is_analysis_run, see there
CLAIM_REFERENCE = 1.12e-14
CLAIM_TOL = 8.0 * CLAIM_REFERENCE


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def same_bits(got, want):
    """the same 64-bit patterns, where a NaN matches any NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.int64), want[ok].view(np.int64))


def exact_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


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


def code_of(csim, call):
    with pytest.raises(csim.CsimError) as info:
        call()
    return info.value.code


# ---- 1. the rows ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", [None, "first", "middle", "last"])
@pytest.mark.parametrize("kind", ["point", "bilinear", "box"])
def test_hold_is_the_operator(csim, kind, where):
    M = 5
    B = M if where is None else M + 1
    t = truth_of(where, B)
    rng = np.random.default_rng([1, B, len(kind)])
    X = members(B, GRID, 1)
    i, j, taps, r = make_network(csim, rng, GRID, kind)
    e = ensemble(csim, X)
    net = e.obs_network(i, j, r, GRID[4], taps=taps)
    assert net.info.nlevels > 1
    net.set_active((np.arange(NOBS) % 3 != 0).astype(np.uint8))   # the mask plays no part
    net.hold(truth_member=t)
    H = net.held()
    assert H.shape == (NOBS, M) and same_bits(H, operator(X, t, i, j, taps).T)
    assert exact_bits(e.download_all(), X)
    e.close()


@pytest.mark.parametrize("M", [2, 5, 65])
@pytest.mark.parametrize("kind", ["point", "box"])
def test_rows_of_other_slots_keep_their_bits(csim, kind, M):
    """65 members cross the 64-lane member loop of the wave that owns an observation"""
    t = 1
    rng = np.random.default_rng([2, M, len(kind)])
    X0, X1 = members(M + 1, GRID, 2), members(M + 1, GRID, 3)
    i, j, taps, r = make_network(csim, rng, GRID, kind)
    slot = rng.integers(0, 3, NOBS)
    slot[:3] = [0, 1, 2]
    e = ensemble(csim, X0)
    net = e.obs_network(i, j, r, GRID[4], taps=taps)
    net.set_slots(slot * 5)                       # slots 0, 5, 10
    net.hold(0, truth_member=t)
    assert code_of(csim, net.held) == ERR_STATE   # 5 and 10 are missing
    e.upload_all(X1)
    net.hold(10, truth_member=t)
    net.hold(5, truth_member=t)
    net.hold(7, truth_member=t)                   # a slot without observations: nothing happens
    H = net.held()
    H0, H1 = operator(X0, t, i, j, taps).T, operator(X1, t, i, j, taps).T
    assert same_bits(H, np.where((slot == 0)[:, None], H0, H1))
    # every observation at once is every slot in turn
    net.hold(truth_member=t)
    assert same_bits(net.held(), H1)
    for s in (0, 5, 10):
        net.hold(s, truth_member=t)
    assert same_bits(net.held(), H1)
    e.close()


# ---- 2. the Gram matrix from one slot's rows is the Gram matrix from the state ---------------------------------------

_cache = {}


def seam_case(nx, ny, M, nobs):
    key = (nx, ny, M, nobs)
    if key not in _cache:
        rng = np.random.default_rng([3, nx, ny, M, nobs])
        X = members(M, (nx, ny), 4)
        i, j = distinct_cells(rng, nx, ny, nobs)
        r = rng.uniform(0.5, 2.0, nobs)
        y = 3.0 + rng.standard_normal(nobs)
        mask = (rng.uniform(size=nobs) < 0.7).astype(np.uint8)
        mask[0] = 0                                # at least one inactive observation
        _cache[key] = (X, i, j, r, y, mask)
    return _cache[key]


def run_one_slot(csim, nx, ny, M, nobs, masked, forms=(0, 1, 2, 3)):
    X, i, j, r, y, mask = seam_case(nx, ny, M, nobs)
    e = ensemble(csim, X, (nx, ny, 1.0, 1.0, 0.4))
    net = e.obs_network(i, j, r, 0.4)
    net.set_values(y)
    if masked:
        net.set_active(mask)
    assert code_of(csim, lambda: e.obs_gram(net, held=True)) == ERR_STATE   # nothing held yet
    net.hold()
    plain = e.obs_gram(net, loglik=True)
    first = None
    for form in forms:
        e.set_option("obs_gram_form", form)
        got = e.obs_gram(net, loglik=True, held=True)
        assert exact_bits(got.A, plain.A) and exact_bits(got.loglik, plain.loglik) and got.n_used == plain.n_used, form
        first = first or got
    e.set_option("obs_gram_form", 0)
    assert plain.n_used == (int(mask.sum()) if masked else nobs)
    bare = e.obs_gram(net, held=True)
    assert bare.loglik is None and exact_bits(bare.A, plain.A)
    # other members: the rows, and so the matrix, keep their bits; the gathering one follows the state
    e.upload_all(members(M, (nx, ny), 5))
    again = e.obs_gram(net, loglik=True, held=True)
    assert exact_bits(again.A, first.A) and exact_bits(again.loglik, first.loglik)
    if plain.n_used:
        assert not exact_bits(e.obs_gram(net).A, first.A)
    e.close()


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("nobs", [1, 63, 64, 65, 129])
def test_held_gram_is_the_gram_at_segment_seams(csim, nobs, masked):
    run_one_slot(csim, 16, 16, 8, nobs, masked)


def test_held_gram_with_256_members(csim):
    run_one_slot(csim, 16, 16, 256, 65, True, forms=(0,))


@pytest.mark.parametrize("kind", ["bilinear", "box"])
def test_held_gram_of_a_linear_network_with_a_truth_member(csim, kind):
    M, t = 12, 4
    rng = np.random.default_rng([4, len(kind)])
    X = members(M + 1, GRID, 6)
    i, j, taps, r = make_network(csim, rng, GRID, kind)
    e = ensemble(csim, X)
    net = e.obs_network(i, j, r, GRID[4], taps=taps)
    net.set_values(3.0 + rng.standard_normal(NOBS))
    mask = np.ones(NOBS, dtype=np.uint8)
    mask[[2, 11, 39]] = 0
    net.set_active(mask)
    net.hold(truth_member=t)
    plain, got = e.obs_gram(net, truth_member=t, loglik=True), e.obs_gram(net, loglik=True, held=True)
    assert got.A.shape == (M + 1, M + 1)
    assert exact_bits(got.A, plain.A) and exact_bits(got.loglik, plain.loglik) and got.n_used == NOBS - 3
    e.close()


def test_masked_rows_are_not_read(csim):
    """a NaN in the row of an inactive observation reaches nothing"""
    M = 6
    X, i, j, r, y, mask = seam_case(16, 16, M, 65)
    X = X.copy()
    o = 0
    assert mask[o] == 0
    X[3, j[o], i[o]] = np.nan
    e = ensemble(csim, X, (16, 16, 1.0, 1.0, 0.4))
    net = e.obs_network(i, j, r, 0.4)
    net.set_values(y)
    net.set_active(mask)
    net.hold()
    assert np.isnan(net.held()[o]).any()
    got = e.obs_gram(net, loglik=True, held=True)
    assert np.isfinite(got.A).all() and np.isfinite(got.loglik).all()
    net.set_active(None)
    assert np.isnan(e.obs_gram(net, held=True).A).any()
    e.close()


# ---- 3. several slots, held from different states ------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["three", "sixty_four"])
def test_gram_of_rows_held_at_different_times(csim, layout):
    M, t = 7, 7
    rng = np.random.default_rng([5, len(layout)])
    X = members(M + 1, GRID, 7)
    if layout == "three":
        nobs = NOBS
        slot = np.where(np.arange(nobs) < 25, 3, 9)   # uneven: 25, 14 and a single observation
        slot[17] = 40
        slot = rng.permutation(slot)
    else:
        nobs = 70
        slot = np.concatenate([np.arange(64), rng.integers(0, 64, 6)])
    i, j, taps, r = make_network(csim, rng, GRID, "box", nobs)
    y = 3.0 + rng.standard_normal(nobs)
    mask = np.ones(nobs, dtype=np.uint8)
    mask[[1, 30]] = 0
    e = ensemble(csim, X, bcs="dnpd")
    e.set_physics(0.05, 0.1, list(np.linspace(-0.5, 0.5, M + 1)), 0.25)
    net = e.obs_network(i, j, r, GRID[4], taps=taps)
    net.set_values(y)
    net.set_active(mask)
    net.set_slots(slot)
    assert csim.obs_slots_present(slot) == held.slots_present(slot)
    states = {}
    for n, s in enumerate(sorted(set(slot.tolist()))):
        if n % 2 == 1:
            e.run(3)
        elif n:
            e.upload_all(members(M + 1, GRID, 100 + n))
        states[s] = e.download_all()
        net.hold(s, truth_member=t)
    H = held.assemble(states, slot, lambda S: operator(S, t, i, j, taps))
    assert same_bits(net.held(), H)
    got = e.obs_gram(net, loglik=True, held=True)
    A, ll, n = ref.obs_gram(H.T, y, r, mask == 1, order_of(csim, net, i, j), loglik=True)
    assert same_bits(got.A, A) and same_bits(got.loglik, ll) and got.n_used == n == nobs - 2
    e.close()


# ---- 4. the analysis -------------------------------------------------------------------------------------------------------

def ring_of(grid):
    ring = np.ones((grid[1] + 2, grid[0] + 2), dtype=bool)
    ring[1:-1, 1:-1] = False
    return ring


ANALYSES = [("point", 5, None, 1.0, False), ("bilinear", 12, "middle", 1.1, False), ("box", 33, "last", 1.0, False),
            ("point", 65, None, 1.1, False), ("point", 8, "first", 1.1, True), ("box", 12, "middle", 1.0, True),
            ("bilinear", 65, "last", 1.1, True)]


@pytest.mark.parametrize("case", ANALYSES, ids=[f"{c[0]}_M{c[1]}_t{c[2]}_lam{c[3]}_{'device' if c[4] else 'host'}"
                                                for c in ANALYSES])
def test_held_analysis_is_the_composition_of_the_public_calls(csim, case):
    kind, M, where, lam, device = case
    B = M if where is None else M + 1
    t = truth_of(where, B)
    rng = np.random.default_rng([6, M])
    X0, X1 = members(B, GRID, 8), members(B, GRID, 9)
    i, j, taps, r = make_network(csim, rng, GRID, kind)
    y = 3.0 + rng.standard_normal(NOBS)
    mask = np.ones(NOBS, dtype=np.uint8)
    mask[[1, 30]] = 0
    slot = rng.integers(0, 2, NOBS)
    a, b = ensemble(csim, X0, bcs="dnpd"), ensemble(csim, X0, bcs="dnpd")
    na, nb = (e.obs_network(i, j, r, GRID[4], taps=taps) for e in (a, b))
    for e, n in ((a, na), (b, nb)):
        n.set_values(y)
        n.set_active(mask)
        n.set_slots(slot)
        n.hold(0, truth_member=t)
        e.upload_all(X1)                      # the state at analysis time is another one than the rows'
        n.hold(1, truth_member=t)
    H = na.held()
    assert same_bits(H, held.assemble({0: X0, 1: X1}, slot, lambda S: operator(S, t, i, j, taps)))
    res = a.assimilate_etkf(na, inflation=lam, truth_member=t, held=True, device=device)
    g = b.obs_gram(nb, held=True)
    w = csim.etkf_weights(g.A, lam, order="round_robin" if device else "rows")
    b.transform(w.W, w.wbar, truth_member=t)
    A, Bc = a.download_all(), b.download_all()
    assert exact_bits(A, Bc) and not exact_bits(A, X1)
    info = a.etkf_info()
    assert info.n_used == g.n_used == NOBS - 2 and exact_bits(info.chi2, g.A[M, M])
    assert exact_bits(info.gamma, w.gamma) and exact_bits(info.dfs, w.dfs)
    if not device:
        assert res.n_used == NOBS - 2 and exact_bits(res.gamma, w.gamma)
    assert np.array_equal(na.status(), np.where(mask == 1, screen.USED, screen.INACTIVE))
    # the members are the transform of the state at analysis time, the rows the same transform of the rows
    assert same_bits(A, espace.transform(X1, w.W, w.wbar, t, True))
    assert same_bits(na.held(), held.row_transform(H, w.W, w.wbar))
    assert exact_bits(A[:, ring_of(GRID)], X1[:, ring_of(GRID)])
    if t is not None:
        assert exact_bits(A[t], X1[t])
    # the window is over
    assert code_of(csim, lambda: a.assimilate_etkf(na, inflation=lam, truth_member=t, held=True, device=device)) == ERR_STATE
    assert code_of(csim, lambda: a.obs_gram(na, held=True)) == ERR_STATE
    assert exact_bits(a.download_all(), A)
    a.close(), b.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_held_just_before_is_the_plain_analysis(csim, device):
    """one slot of point observations held immediately before: the plain ETKF's members, and the transformed rows are
    the analysed members at the observed cells"""
    M, t, lam = 9, 3, 1.05
    rng = np.random.default_rng(7)
    X = members(M + 1, GRID, 10)
    i, j, _, r = make_network(csim, rng, GRID, "point")
    y = 3.0 + rng.standard_normal(NOBS)
    a, b = ensemble(csim, X), ensemble(csim, X)
    na, nb = (e.obs_network(i, j, r, GRID[4]) for e in (a, b))
    na.set_values(y), nb.set_values(y)
    na.hold(truth_member=t)
    a.assimilate_etkf(na, inflation=lam, truth_member=t, held=True, device=device)
    b.assimilate_etkf(nb, inflation=lam, truth_member=t, device=device)
    A = a.download_all()
    assert exact_bits(A, b.download_all()) and not exact_bits(A, X)
    assert exact_bits(na.held(), operator(A, t, i, j, None).T)
    ia, ib = a.etkf_info(), b.etkf_info()
    assert ia.n_used == ib.n_used and exact_bits(ia.chi2, ib.chi2) and exact_bits(ia.gamma, ib.gamma)
    a.close(), b.close()


# ---- 5. the screening and the record come from the rows ----------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_screen_and_record_from_the_rows(csim, device):
    M, t, tol, lam = 9, 0, 3.0, 1.05
    rng = np.random.default_rng(8)
    X0, X1 = members(M + 1, GRID, 11), members(M + 1, GRID, 12)
    i, j, taps, r = make_network(csim, rng, GRID, "bilinear")
    H = operator(X0, t, i, j, taps).T
    hb, vb = held.row_mv(H)
    y = hb + 0.5 * np.sqrt(vb + r) * rng.standard_normal(NOBS).clip(-2, 2)
    y[8] = hb[8] + 50.0 * np.sqrt(vb[8] + r[8])     # a gross error against the rows, not against the state
    y[21] = hb[21] - 40.0 * np.sqrt(vb[21] + r[21])
    mask = np.ones(NOBS, dtype=np.uint8)
    mask[[3, 12, 20]] = 0
    st = screen.statuses(y, hb, vb, r, tol, mask)
    assert st[8] == st[21] == screen.REJECTED and set(st.tolist()) == {0, 1, 2}
    e = ensemble(csim, X0)
    net = e.obs_network(i, j, r, GRID[4], taps=taps, log_cycles=2)
    net.set_values(y)
    net.set_active(mask)
    net.hold(truth_member=t)
    assert same_bits(net.held(), H)
    e.upload_all(X1)
    e.assimilate_etkf(net, inflation=lam, truth_member=t, record=True, screen=tol, held=True, device=device)
    assert np.array_equal(net.status(), st)
    info = e.etkf_info()
    assert info.n_used == np.count_nonzero(st == screen.USED)
    A = ref.obs_gram(H.T, y, r, st == screen.USED, order_of(csim, net, i, j))[0]
    w = csim.etkf_weights(A, lam, order="round_robin" if device else "rows")
    Ha = held.row_transform(H, w.W, w.wbar)
    assert same_bits(net.held(), Ha)
    assert same_bits(e.download_all(), espace.transform(X1, w.W, w.wbar, t, True))
    ha, va = held.row_mv(Ha)
    f = net.fetch()
    assert same_bits(f.bg_mean, hb) and same_bits(f.bg_var, vb) and same_bits(f.post_mean, ha) and same_bits(f.post_var, va)
    log, slog = net.log(), net.screen_log()
    assert len(log) == 1 and len(slog) == 1
    rec, srec = screen.cycle(y, hb, vb, ha, va, r, st), screen.screen_cycle(st)
    assert all(exact_bits(log[0][k], rec[k]) for k in obsnet.FIELDS), (log[0], rec)
    assert all(exact_bits(slog[0][k], srec[k]) for k in screen.SCREEN_FIELDS), (slog[0], srec)
    # forecast impact for held observations is not built, and says so
    with pytest.raises(csim.CsimError) as ei:
        net.impact_capture(truth_member=t)
    assert ei.value.code == ERR_STATE and "held" in str(ei.value)
    # a plain recorded analysis afterwards is captured as ever
    e.assimilate_etkf(net, truth_member=t, record=True)
    net.impact_capture(truth_member=t)
    e.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_nothing_used_and_no_inflation_keeps_every_bit(csim, device):
    M = 6
    rng = np.random.default_rng(9)
    X0, X1 = members(M, GRID, 13), members(M, GRID, 14)
    i, j, _, r = make_network(csim, rng, GRID, "point")
    e = ensemble(csim, X0)
    net = e.obs_network(i, j, r, GRID[4])
    net.set_values(rng.standard_normal(NOBS))
    net.set_active(np.zeros(NOBS, dtype=np.uint8))
    net.hold()
    H = net.held()
    e.upload_all(X1)
    e.assimilate_etkf(net, held=True, device=device)
    info = e.etkf_info()
    assert info.n_used == 0 and info.chi2 == 0.0
    assert exact_bits(e.download_all(), X1) and exact_bits(net.held(), H)
    assert (net.status() == screen.INACTIVE).all()
    # with inflation the rows spread as the members do
    net.hold()
    H1 = net.held()
    e.assimilate_etkf(net, inflation=1.1, held=True, device=device)
    w = csim.etkf_weights(np.zeros((M + 1, M + 1)), 1.1, order="round_robin" if device else "rows")
    assert same_bits(net.held(), held.row_transform(H1, w.W, w.wbar)) and not exact_bits(net.held(), H1)
    e.close()


# ---- 6. observe by slot ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["point", "box"])
def test_observe_slot(csim, kind):
    B, s = 5, 2
    rng = np.random.default_rng([10, len(kind)])
    X0, X1 = members(B, GRID, 15), members(B, GRID, 16)
    i, j, taps, r = make_network(csim, rng, GRID, kind)
    slot = rng.integers(0, 3, NOBS) * 31           # slots 0, 31, 62
    slot[:3] = [0, 31, 62]
    e, whole = ensemble(csim, X0), ensemble(csim, X0)
    net, wnet = (x.obs_network(i, j, r, GRID[4], taps=taps) for x in (e, whole))
    net.set_slots(slot)
    wnet.observe(s, seed=11, draw=3)
    w0 = wnet.fetch()
    net.observe(s, seed=11, draw=3, slot=31)
    assert code_of(csim, lambda: e.obs_gram(net)) == ERR_STATE        # no values before every slot is observed
    assert net.fetch().y is None
    net.observe(s, seed=11, draw=3, slot=0)
    e.upload_all(X1), whole.upload_all(X1)
    wnet.observe(s, seed=11, draw=3)
    w1 = wnet.fetch()
    net.observe(s, seed=11, draw=3, slot=62)
    f = net.fetch()
    late = slot == 62
    assert exact_bits(f.y, np.where(late, w1.y, w0.y)) and exact_bits(f.truth, np.where(late, w1.truth, w0.truth))
    assert not exact_bits(w0.y, w1.y)
    assert e.obs_gram(net).n_used == NOBS
    # without noise the values are the truth
    net.observe(s, seed=11, noise=False, slot=31)
    g = net.fetch()
    mid = slot == 31
    assert exact_bits(g.y[mid], w1.truth[mid]) and exact_bits(g.y[~mid], f.y[~mid])
    # values from the host end the truth, and the slots start again
    net.set_values(f.y)
    net.observe(s, seed=11, slot=0)
    assert net.fetch().truth is None
    e.close(), whole.close()


# ---- 7. errors and state ---------------------------------------------------------------------------------------------------

def test_errors_and_state(csim):
    rng = np.random.default_rng(12)
    grid = (8, 8, 1.0, 1.0, 2.5)
    X = members(4, grid, 17)
    i, j, r = np.array([2, 5, 7], dtype=np.int32), np.array([3, 6, 1], dtype=np.int32), np.array([1.0, 0.5, 2.0])
    e, other = ensemble(csim, X, grid), ensemble(csim, X, grid)
    net = e.obs_network(i, j, r, 2.5, log_cycles=1)
    # a slot out of range, before anything changes
    for bad in ([0, 1, 64], [-1, 0, 0]):
        assert code_of(csim, lambda: net.set_slots(bad)) == ERR_ARG
    with pytest.raises(ValueError):
        net.set_slots([0, 1])
    for bad in (-2, 64):
        assert code_of(csim, lambda: net.hold(bad)) == ERR_ARG
        assert code_of(csim, lambda: net.observe(0, seed=1, slot=bad)) == ERR_ARG
    assert code_of(csim, lambda: net.hold(0, truth_member=4)) == ERR_ARG
    net.hold()
    # no values yet
    assert code_of(csim, lambda: e.obs_gram(net, held=True)) == ERR_STATE
    assert code_of(csim, lambda: e.assimilate_etkf(net, held=True)) == ERR_STATE
    net.set_values(rng.standard_normal(3))
    assert e.obs_gram(net, held=True).n_used == 3
    # a network of another ensemble
    assert code_of(csim, lambda: other.obs_gram(net, held=True)) == ERR_ARG
    assert code_of(csim, lambda: other.assimilate_etkf(net, held=True)) == ERR_ARG
    # set_slots forgets the holds; a slot missing
    net.set_slots([0, 1, 1])
    assert code_of(csim, net.held) == ERR_STATE
    net.hold(1)
    for call in (net.held, lambda: e.obs_gram(net, held=True), lambda: e.assimilate_etkf(net, held=True),
                 lambda: e.assimilate_etkf(net, held=True, device=True)):
        assert code_of(csim, call) == ERR_STATE
    net.hold(0)
    assert net.held().shape == (3, 4)
    # the analysis's own errors come first, then a truth member that differs from the hold's
    assert code_of(csim, lambda: e.assimilate_etkf(net, held=True, inflation=0.5)) == ERR_ARG
    assert code_of(csim, lambda: e.assimilate_etkf(net, held=True, truth_member=4)) == ERR_ARG
    assert code_of(csim, lambda: e.assimilate_etkf(net, held=True, truth_member=2)) == ERR_STATE
    assert exact_bits(e.download_all(), X)
    # a hold with another truth member forgets the rows held so far
    net.hold(0, truth_member=2)
    assert code_of(csim, net.held) == ERR_STATE
    net.hold(1, truth_member=2)
    assert net.held().shape == (3, 3)
    e.assimilate_etkf(net, held=True, truth_member=2, record=True)
    assert code_of(csim, lambda: e.assimilate_etkf(net, held=True, truth_member=2)) == ERR_STATE   # no new holds
    assert net.held().shape == (3, 3)                                                               # the analysed rows
    assert code_of(csim, lambda: net.impact_capture(truth_member=2)) == ERR_STATE
    net.hold(0, truth_member=2)
    assert code_of(csim, net.held) == ERR_STATE
    # M = 1 and M = 257
    two = ensemble(csim, X[:2], grid)
    n2 = two.obs_network(i, j, r, 2.5)
    assert code_of(csim, lambda: n2.hold(truth_member=0)) == ERR_UNSUPPORTED
    n2.hold()
    assert n2.held().shape == (3, 2)
    big = csim.Ensemble(258, 4, 4, 1.0, 1.0, csim.bc_codes("dddd"), 0.5)
    nb = big.obs_network([2], [2], [1.0], 2.5)
    assert code_of(csim, nb.hold) == ERR_UNSUPPORTED
    assert code_of(csim, lambda: nb.hold(truth_member=0)) == ERR_UNSUPPORTED
    L = csim.lib()
    assert L.csim_obs_network_hold(None, 0, -1) == ERR_ARG
    assert L.csim_obs_network_set_slots(None, None) == ERR_ARG
    assert L.csim_obs_network_held(None, None, None, None) == ERR_ARG
    assert L.csim_ensemble_obs_gram_held(None, None, None, None, None) == ERR_ARG
    assert L.csim_ensemble_assimilate_etkf_held(None, None, 1.0, -1, 0, 0.0, 0) == ERR_ARG
    assert L.csim_ensemble_assimilate_etkf_held(e._h, net._h, 1.0, 2, 0, 0.0, 2) == ERR_ARG
    for x in (e, other, two, big):
        x.close()


# ---- 8. the claim ------------------------------------------------------------------------------------------------------------

def test_hold_run_analysis_is_analysis_run(csim):
    """The model is affine and one physics is common to the members, so holding at t1, running n steps and analysing
    with the held rows gives, up to rounding, the members of analysing at t1 and running the same n steps.

    The tolerance is measured, not tuned: tests/test_held_host.py walks both paths in numpy (the oracle's stepping, the
    restatements of the Gram matrix, the weights and the transform) over the 32 seeded scenarios of
    held_restatement.claim_scenarios (seed s: kind point / bilinear / box by s % 3, M = 5, 8, 12, 33 by s % 4, inflation
    1.0 / 1.1 by (s // 2) % 2, sides dddd / dnnd by (s // 4) % 2; 37 x 21 cells, 40 observations, D = 0.05, dt = 0.4,
    v = (1.0, 0.5), n = 10 steps, so a feature moves 4 cells along x and 2 along y).  Its largest difference relative
    to the RMS analysis increment is 1.117e-14 (CLAIM_REFERENCE, rounded up to 1.12e-14); the GPU may differ by 8 times
    that, the margin of the forecast-impact test for the same kind of claim: other, equally valid summation orders.
    In every scenario the plain analysis at t1 + n, whose rows come from the wrong time, must differ from the second
    path by more than 100 times the tolerance (on the CPU it differs by 2.5 to 7 increments), else the test shows
    nothing.  The periodic sides are left out: a periodic ghost cell is part of the state at the first step of a run,
    and a transform leaves the ghost ring alone."""
    D, dt, vx, vy = held.CLAIM_PHYSICS
    worst, least = 0.0, np.inf
    for sc in held.claim_scenarios():
        seed, kind, M, lam, bcs = sc
        X1, i, j, taps, r, z = held.claim_case(csim, sc)
        t = M
        y = operator(X1, None, i, j, taps)[t] + np.sqrt(r) * z
        ens = [ensemble(csim, X1, held.CLAIM_GRID, bcs) for _ in range(4)]
        nets = [e.obs_network(i, j, r, held.CLAIM_GRID[4], taps=taps) for e in ens]
        for e, n in zip(ens, nets):
            e.set_physics(D, dt, vx, vy)
            n.set_values(y)
        one, two, wrong, free = ens
        nets[0].hold(truth_member=t)
        one.run(held.CLAIM_STEPS)
        one.assimilate_etkf(nets[0], inflation=lam, truth_member=t, held=True)
        two.assimilate_etkf(nets[1], inflation=lam, truth_member=t)
        two.run(held.CLAIM_STEPS)
        wrong.run(held.CLAIM_STEPS)
        wrong.assimilate_etkf(nets[2], inflation=lam, truth_member=t)
        free.run(held.CLAIM_STEPS)
        A, B, Wr, F = (e.download_all() for e in ens)
        err, off = held.claim_error(A, B, F, M), held.claim_error(Wr, B, F, M)
        print(f"scenario {sc}: held path against analysis first {err:.3e}, rows from the wrong time {off:.3e}")
        worst, least = max(worst, err), min(least, off)
        for e in ens:
            e.close()
    print(f"largest {worst:.3e} (allowed {CLAIM_TOL:.3e}), least wrong-time difference {least:.3e}")
    assert least > 100.0 * CLAIM_TOL
    assert worst <= CLAIM_TOL
