"""Screening of observation networks on the GPU (csim_obs_network_set_active, csim_ensemble_assimilate_screened,
csim_obs_network_status, csim_obs_network_screen_log), bit for bit: nothing screened against the unscreened call; a
screened analysis against the unscreened analysis of the USED observations (ordered = 1) and against the numpy
restatement with the full plan's levels (ordered = 0); statuses, both logs and the diagnostics against
tests/screen_restatement.py (pinned by tests/test_ensemble_screen_host.py); an unrecorded screened analysis; the whole
cycle enqueued; stepping parity; errors; an OSSE with corrupted reports.  The grids are small: what is under test goes
per observation and per window, not per grid."""
import numpy as np
import pytest

import obsnet_restatement as obsnet
import obsop_restatement as obsop
import screen_restatement as ref
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

# nx, ny, dx, dy, loc: windows of 7 x 9 and 7 x 7 cells, so that levels and clipped windows both occur
GRIDS = [(40, 28, 1.0, 0.8, 2.0), (33, 17, 1.0, 1.25, 2.0)]
TOL = 4.0


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    for nx, ny, dx, dy, loc in GRIDS:
        tab = pkg.ensemble_gc_table(dx, dy, loc, nx, ny)
        assert 2 <= tab.shape[0] // 2 <= 4 and 2 <= tab.shape[1] // 2 <= 4
    return pkg


def same_bits(got, want):
    """the same 64-bit patterns, where a NaN matches any NaN (as in tests/test_gpu_ensemble_assim.py)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.int64), want[ok].view(np.int64))


def exact_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def log_matches(row, rec, fields):
    return all(exact_bits(row[f], rec[f]) for f in fields)


PHYS = [(0.05, 0.1, 0.5, -0.25), (0.02, 0.1, -0.3, 0.4), (0.08, 0.05, 0.0, 0.0), (0.01, 0.1, 0.2, 0.2),
        (0.03, 0.1, -0.2, -0.1)]


def physics(B):
    return [[PHYS[m % len(PHYS)][k] for m in range(B)] for k in range(4)]


def ensemble(csim, X, grid, bcs="dddd"):
    nx, ny, dx, dy, _ = grid
    e = csim.Ensemble(X.shape[0], nx, ny, dx, dy, csim.bc_codes(bcs), 0.5)
    e.upload_all(X)
    e.set_physics(*physics(X.shape[0]))
    return e


def make_network(csim, rng, grid, kind, nobs):
    """(i, j, taps or None, r): point observations with corners, edges and a duplicated cell; bilinear stations between
    grid points; 3 x 3 footprints clipped at the sides.  The first three observations are a chain A - B - C along x, A
    and C two windows apart: B conflicts with both, they do not conflict with each other"""
    nx, ny, dx, dy, loc = grid
    tab = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    lx = tab.shape[1] // 2
    if kind == "bilinear":
        x, y = rng.uniform(1, nx, nobs), rng.uniform(1, ny, nobs)
        if nobs >= 3:
            x[:3], y[:3] = [5.5, 5.5 + 2 * lx, 5.5 + 4 * lx], [10.25, 10.25, 10.25]
        i, j, taps = csim.bilinear_taps(nx, ny, x, y)
        return i, j, tuple(taps), rng.uniform(0.05, 2.0, nobs)
    i, j = rng.integers(1, nx + 1, nobs), rng.integers(1, ny + 1, nobs)
    if nobs >= 3:
        i[:3], j[:3] = [5, 5 + 2 * lx, 5 + 4 * lx], [10, 10, 10]
    if nobs >= 12:
        i[3:9] = [1, nx, 1, nx, 1, (nx + 1) // 2]
        j[3:9] = [1, ny, ny, 1, (ny + 1) // 2, 1]
        i[9], j[9] = i[3], j[3]
    i, j = i.astype(np.int32), j.astype(np.int32)
    if kind == "box":
        i, j, taps = csim.box_taps(nx, ny, i, j, 1, 1)
        return i, j, tuple(taps), rng.uniform(0.05, 2.0, nobs)
    return i, j, None, rng.uniform(0.05, 2.0, nobs)


def background(X, t, i, j, taps):
    """(hb, vb) of the definition's step 1, on the CPU"""
    return obsnet.mv(X, t, i, j) if taps is None else obsop.mv(X, t, i, j, taps)


def screened_values(rng, hb, vb, r, active_share=0.5, corrupt=4):
    """values well inside the check (half a standard deviation of the innovation), `corrupt` of them moved out by 50
    standard deviations, and a mask of about active_share ones: at least one corrupted observation is active, at least
    one is not, so that with tol = TOL all three statuses occur by construction.  Inactive ones get NaN-free garbage"""
    n = len(hb)
    sd = np.sqrt(vb + r)
    y = hb + 0.5 * sd * rng.standard_normal(n).clip(-2, 2)
    mask = (rng.uniform(size=n) < active_share).astype(np.uint8)
    bad = rng.permutation(n)[:min(corrupt, n)]
    y[bad] = hb[bad] + 50.0 * sd[bad] * np.where(rng.uniform(size=len(bad)) < 0.5, -1.0, 1.0)
    if n >= 3:
        mask[bad[0]] = 1
        mask[bad[1]] = 0
        good = np.setdiff1d(np.arange(n), bad)
        mask[good[0]] = 1
    return y, mask, bad


def subset_taps(taps, keep):
    start, di, dj, w = taps
    return obsop.concat([(list(di[start[o]:start[o + 1]]), list(dj[start[o]:start[o + 1]]),
                          list(w[start[o]:start[o + 1]])) for o in keep])


def ring_of(X):
    ring = np.ones(X.shape[1:], dtype=bool)
    ring[1:-1, 1:-1] = False
    return ring


# ---- 1. nothing screened: the unscreened analysis --------------------------------------------------------------------

# every M (2: the least; 5; 64: the widest register form of the update; 65: the re-read form) with every kind of
# network; truth member and inflation rotated so that each meets both values
IDENTITY = [(M, kind, (a + b) % 2 == 0, [1.0, 1.05][(a + b // 2) % 2], GRIDS[(a + b) % 2])
            for a, M in enumerate((2, 5, 64, 65)) for b, kind in enumerate(("point", "bilinear", "box"))]


@pytest.mark.parametrize("case", IDENTITY, ids=[f"M{c[0]}_{c[1]}_t{int(c[2])}_lam{c[3]}_{c[4][0]}x{c[4][1]}"
                                                for c in IDENTITY])
def test_nothing_screened_is_the_unscreened_analysis(csim, case):
    """a mask of ones and a tolerance under which the restatement rejects nothing, against assimilate_network on a twin:
    members with ghosts, and again after a run (which reads the other ping-pong buffer), the log record, the statuses"""
    M, kind, with_truth, lam, grid = case
    nx, ny, dx, dy, loc = grid
    B = M + 1 if with_truth else M
    t = B // 2 if with_truth else None
    rng = np.random.default_rng(100 * M + len(kind))
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, taps, r = make_network(csim, rng, grid, kind, 40)
    y = rng.standard_normal(40)
    a, b = ensemble(csim, X, grid), ensemble(csim, X, grid)
    nets = []
    for e in (a, b):
        e.run(2)
        net = e.obs_network(i, j, r, loc, log_cycles=2, taps=taps)
        net.set_values(y)
        nets.append(net)
    before = a.download_all()
    na, nb = nets
    na.set_active(np.ones(40, dtype=np.uint8))
    a.assimilate_network(na, inflation=lam, truth_member=t, record=True, screen=1e6)
    b.assimilate_network(nb, inflation=lam, truth_member=t, record=True)
    A, W = a.download_all(), b.download_all()
    assert same_bits(A, W) and not same_bits(A, before)
    fa, fb = na.fetch(), nb.fetch()
    assert not ref.statuses(y, fa.bg_mean, fa.bg_var, r, 1e6).any()
    for k in ("bg_mean", "bg_var", "post_mean", "post_var"):
        assert same_bits(getattr(fa, k), getattr(fb, k)), k
    assert na.log().tobytes() == nb.log().tobytes() and len(na.log()) == 1
    for net in nets:
        assert net.screen_log().tolist() == [(40.0, 0.0, 0.0)]
        assert net.status().dtype == np.uint8 and not net.status().any()
    assert na.log()["n"][0] == 40.0
    a.run(3), b.run(3)
    assert same_bits(a.download_all(), b.download_all())
    a.close(), b.close()


# ---- 2. ordered: the unscreened analysis of the USED observations -----------------------------------------------------

SUBSET = [(5, "point", True, 1.05, GRIDS[0]), (64, "point", False, 1.0, GRIDS[1]), (65, "point", True, 1.0, GRIDS[0]),
          (2, "bilinear", False, 1.05, GRIDS[1]), (64, "box", True, 1.05, GRIDS[0]), (65, "bilinear", False, 1.0, GRIDS[1])]
IDS = [f"M{c[0]}_{c[1]}_t{int(c[2])}_lam{c[3]}_{c[4][0]}x{c[4][1]}" for c in SUBSET]


@pytest.mark.parametrize("case", SUBSET, ids=IDS)
def test_ordered_subset_is_the_analysis_of_the_subset(csim, case):
    """ordered = 1, about half the observations masked out and four values moved 50 standard deviations away: members
    bit for bit those of csim_ensemble_assimilate (point) or of a fresh linear network (linear) given the USED
    observations only; statuses those of the restatement from the fetched (hb, vb)"""
    M, kind, with_truth, lam, grid = case
    nx, ny, dx, dy, loc = grid
    B = M + 1 if with_truth else M
    t = B // 2 if with_truth else None
    rng = np.random.default_rng(200 * M + len(kind))
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, taps, r = make_network(csim, rng, grid, kind, 40)
    hb, vb = background(X, t, i, j, taps)
    y, mask, bad = screened_values(rng, hb, vb, r)
    want_st = ref.statuses(y, hb, vb, r, TOL, mask)
    assert set(want_st.tolist()) == {0, 1, 2}, "the case must screen: all three statuses"
    a, b = ensemble(csim, X, grid), ensemble(csim, X, grid)
    net = a.obs_network(i, j, r, loc, ordered=True, log_cycles=1, taps=taps)
    yy = y.copy()
    yy[mask == 0] = 1e30          # never looked at
    net.set_values(yy)
    net.set_active(mask)
    a.assimilate_network(net, inflation=lam, truth_member=t, record=True, screen=TOL)
    st, f = net.status(), net.fetch()
    assert same_bits(f.bg_mean, hb) and same_bits(f.bg_var, vb)
    assert np.array_equal(st, ref.statuses(yy, f.bg_mean, f.bg_var, r, TOL, mask)) and np.array_equal(st, want_st)
    assert (st[bad[mask[bad] == 1]] == ref.REJECTED).all()
    keep = np.flatnonzero(st == ref.USED)
    if taps is None:
        b.assimilate(i[keep], j[keep], y[keep], r[keep], loc, inflation=lam, truth_member=t, ordered=True,
                     diagnostics=False)
    else:
        sub = b.obs_network(i[keep], j[keep], r[keep], loc, ordered=True, taps=subset_taps(taps, keep))
        sub.set_values(y[keep])
        b.assimilate_network(sub, inflation=lam, truth_member=t)
    A, W = a.download_all(), b.download_all()
    assert same_bits(A, W) and not same_bits(A, X)
    assert exact_bits(A[:, ring_of(X)], X[:, ring_of(X)])
    if t is not None:
        assert exact_bits(A[t], X[t])
    ha, va = background(A, t, i, j, taps)
    assert same_bits(f.post_mean, ha) and same_bits(f.post_var, va)     # every observation, whatever its status
    a.run(3), b.run(3)
    assert same_bits(a.download_all(), b.download_all())
    a.close(), b.close()


# ---- 3. not ordered: the order of the full plan ------------------------------------------------------------------------

@pytest.mark.parametrize("case", SUBSET[:2] + SUBSET[3:5], ids=IDS[:2] + IDS[3:5])
def test_full_plan_order(csim, case):
    """ordered = 0: against the restatement's filter over the USED observations with the levels of the full plan.  A is
    inactive, B and C are used: the full plan has C (level 0, beside A) before B (level 1), a first-fit plan of the
    subset has B before C, and the two orders give other bits, so an implementation that plans again fails here"""
    M, kind, with_truth, lam, grid = case
    nx, ny, dx, dy, loc = grid
    B = M + 1 if with_truth else M
    t = B // 2 if with_truth else None
    rng = np.random.default_rng(300 * M + len(kind))
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, taps, r = make_network(csim, rng, grid, kind, 40)
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    ly, lx = rho.shape[0] // 2, rho.shape[1] // 2
    lev = csim.ensemble_assim_plan(i, j, lx, ly, False)
    hb, vb = background(X, t, i, j, taps)
    y, mask, bad = screened_values(rng, hb, vb, r)
    for o in range(3):               # the chain: good values, A masked out
        y[o] = hb[o] + 0.5 * np.sqrt(vb[o] + r[o])
    mask[:3] = [0, 1, 1]
    want_st = ref.statuses(y, hb, vb, r, TOL, mask)
    assert set(want_st.tolist()) == {0, 1, 2} and want_st[:3].tolist() == [1, 0, 0]
    keep = np.flatnonzero(want_st == ref.USED)
    sub_lev = csim.ensemble_assim_plan(i[keep], j[keep], lx, ly, False)
    assert lev[2] < lev[1] and sub_lev[0] < sub_lev[1] and keep[:2].tolist() == [1, 2]
    full_taps = taps if taps is not None else ref.point_taps(40)
    want = ref.subset_analysis(X, rho, lev, i, j, full_taps, y, r, lam, t, want_st)
    replanned = obsop.analysis(X, rho, sub_lev, i[keep], j[keep], subset_taps(full_taps, keep), y[keep], r[keep], lam, t)
    assert not same_bits(want, replanned)
    e = ensemble(csim, X, grid)
    net = e.obs_network(i, j, r, loc, ordered=False, taps=taps)
    assert net.info.nlevels == lev.max() + 1
    net.set_values(y)
    net.set_active(mask)
    e.assimilate_network(net, inflation=lam, truth_member=t, screen=TOL)
    A = e.download_all()
    assert np.array_equal(net.status(), want_st)
    assert same_bits(A, want) and not same_bits(A, replanned)
    e.close()


# ---- 4. the logs -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nobs", [1, 255, 256, 257, 1500])
def test_logs_and_diagnostics(csim, nobs):
    """three recorded cycles on an ordered point network (mask and rejections with a truth; everything inactive with
    inflation; everything inactive without): both logs against the restatement bit for bit, the diagnostics present
    for every observation, the members against csim_ensemble_assimilate of the USED ones and the inflation alone"""
    grid = GRIDS[0]
    nx, ny, dx, dy, loc = grid
    B, t = 7, 2
    rng = np.random.default_rng(nobs)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, _, r = make_network(csim, rng, grid, "point", nobs)
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    a, b = ensemble(csim, X, grid), ensemble(csim, X, grid)
    net = a.obs_network(i, j, r, loc, ordered=True, log_cycles=3)
    # cycle 0: observed from the truth member, then screened with a mask
    net.observe(t, 9, 0)
    y, xt = obsnet.observe(X, t, i, j, r, 9, 0, True)
    hb, vb = obsnet.mv(X, t, i, j)
    mask = (rng.uniform(size=nobs) < 0.6).astype(np.uint8)
    mask[0] = 1
    st = ref.statuses(y, hb, vb, r, 1.5, mask)   # a tight check: good observations are rejected too
    if nobs > 1:
        assert set(st.tolist()) == {0, 1, 2}
    net.set_active(mask)
    a.assimilate_network(net, inflation=1.05, truth_member=t, record=True, screen=1.5)
    keep = np.flatnonzero(st == 0)
    if len(keep):
        b.assimilate(i[keep], j[keep], y[keep], r[keep], loc, inflation=1.05, truth_member=t, ordered=True,
                     diagnostics=False)
        W = b.download_all()
    else:   # the inflation alone
        W = ref.subset_analysis(X, rho, np.zeros(nobs, dtype=np.int32), i, j, ref.point_taps(nobs), y, r, 1.05, t, st)
    A = a.download_all()
    assert same_bits(A, W)
    f = net.fetch()
    ha, va = obsnet.mv(A, t, i, j)
    assert np.array_equal(net.status(), st)
    assert same_bits(f.bg_mean, hb) and same_bits(f.bg_var, vb) and same_bits(f.post_mean, ha) and same_bits(f.post_var, va)
    want = [(ref.cycle(y, hb, vb, ha, va, r, st, xt), ref.screen_cycle(st))]
    # cycle 1: everything inactive, inflation alone; the values are kept
    net.set_active(np.zeros(nobs, dtype=np.uint8))
    a.assimilate_network(net, inflation=1.1, truth_member=t, record=True, screen=1.5)
    hb, vb = obsnet.mv(A, t, i, j)
    A1 = a.download_all()
    none = np.full(nobs, ref.INACTIVE)
    assert same_bits(A1, ref.subset_analysis(A, rho, np.zeros(nobs, dtype=np.int32), i, j, ref.point_taps(nobs), y, r,
                                             1.1, t, none))
    assert not same_bits(A1, A) and np.array_equal(net.status(), none)
    ha, va = obsnet.mv(A1, t, i, j)
    f = net.fetch()
    assert same_bits(f.bg_mean, hb) and same_bits(f.post_mean, ha) and same_bits(f.post_var, va)
    want.append((ref.cycle(y, hb, vb, ha, va, r, none, xt), ref.screen_cycle(none)))
    # cycle 2: the same without inflation and without a check: nothing changes, in either buffer
    a.assimilate_network(net, truth_member=t, record=True)
    assert exact_bits(a.download_all(), A1)
    want.append((ref.cycle(y, ha, va, ha, va, r, none, xt), ref.screen_cycle(none)))
    log, slog = net.log(), net.screen_log()
    assert len(log) == 3 and len(slog) == 3
    for c, (rec, srec) in enumerate(want):
        assert log_matches(log[c], rec, obsnet.FIELDS), (c, log[c], rec)
        assert log_matches(slog[c], srec, ref.SCREEN_FIELDS), (c, slog[c], srec)
        assert log[c]["n"] == slog[c]["n_used"]
        assert slog[c]["n_used"] + slog[c]["n_inactive"] + slog[c]["n_rejected"] == nobs
    for c in (1, 2):
        assert log[c]["n"] == 0.0 and slog[c]["n_inactive"] == nobs
        assert all(log[c][k] == 0.0 and not np.signbit(log[c][k]) for k in obsnet.FIELDS[2:])
    b.close()
    b = ensemble(csim, A1, grid)
    a.run(3), b.run(3)
    assert same_bits(a.download_all(), b.download_all())
    # log_reset resets both logs; a cycle that is not screened leaves (nobs, 0, 0) in the second
    net.log_reset()
    assert len(net.log()) == 0 and len(net.screen_log()) == 0
    net.set_active(None)
    a.assimilate_network(net, truth_member=t, record=True)
    assert net.screen_log().tolist() == [(float(nobs), 0.0, 0.0)] and net.log()["n"][0] == nobs
    assert not net.status().any()
    a.close(), b.close()


# ---- 5. an unrecorded screened analysis ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["point", "box"])
def test_unrecorded_screened_analysis_keeps_the_recorded_diagnostics(csim, kind):
    grid = GRIDS[1]
    nx, ny, dx, dy, loc = grid
    rng = np.random.default_rng(55)
    X = rng.standard_normal((6, ny + 2, nx + 2))
    i, j, taps, r = make_network(csim, rng, grid, kind, 40)
    e = ensemble(csim, X, grid)
    net = e.obs_network(i, j, r, loc, ordered=True, log_cycles=2, taps=taps)
    hb, vb = background(X, None, i, j, taps)
    y, mask, _ = screened_values(rng, hb, vb, r)
    net.set_values(y)
    net.set_active(mask)
    e.assimilate_network(net, record=True, screen=TOL)
    first, st1, A = net.fetch(), net.status(), e.download_all()
    assert np.array_equal(st1, ref.statuses(y, hb, vb, r, TOL, mask))
    hb2, vb2 = background(A, None, i, j, taps)
    assert not same_bits(hb2, hb)
    y2, mask2, _ = screened_values(rng, hb2, vb2, r)
    net.set_values(y2)
    net.set_active(mask2)
    e.assimilate_network(net, screen=TOL)          # not recorded
    st2, second = net.status(), net.fetch()
    want2 = ref.statuses(y2, hb2, vb2, r, TOL, mask2)
    assert np.array_equal(st2, want2) and not np.array_equal(st2, st1) and set(want2.tolist()) == {0, 1, 2}
    for k in ("bg_mean", "bg_var", "post_mean", "post_var"):
        assert exact_bits(getattr(second, k), getattr(first, k)), k
    assert exact_bits(second.y, y2) and len(net.log()) == 1 and len(net.screen_log()) == 1
    assert not same_bits(e.download_all(), A)
    e.close()


# ---- 6. the whole cycle, enqueued ---------------------------------------------------------------------------------------

def test_whole_screened_cycle_enqueued(csim):
    """three cycles of run -> observe -> set_active -> prior_capture -> assimilate_network(screen, record) -> relax ->
    perturb with no synchronising call in between, then one log, screen_log and status: the same as with a sync after
    every call"""
    grid = GRIDS[0]
    nx, ny, dx, dy, loc = grid
    B, seed = 9, 77
    rng = np.random.default_rng(6)
    X = 0.2 * rng.standard_normal((B, ny + 2, nx + 2))
    X[0] += 1.0   # the truth lies apart from the forecast: with tol = 1 some observations are rejected
    i, j, _, r = make_network(csim, rng, grid, "point", 60)
    masks = [(rng.uniform(size=60) < 0.7).astype(np.uint8) for _ in range(3)]
    got = []
    for form in ("enqueued", "synced"):
        e = ensemble(csim, X, grid, "dnpd")
        net = e.obs_network(i, j, r, loc, log_cycles=3)
        for cyc in range(3):
            steps = [lambda: e.run(3), lambda: net.observe(0, seed, cyc), lambda: net.set_active(masks[cyc]),
                     lambda: e.prior_capture("spread", truth_member=0),
                     lambda: e.assimilate_network(net, truth_member=0, record=True, screen=1.0),
                     lambda: e.relax(0.6, truth_member=0),
                     lambda: e.perturb(0.05, 3.0, seed, cyc, centered=True, truth_member=0)]
            for step in steps:
                step()
                if form == "synced":
                    e.sync()
        got.append((net.log(), net.screen_log(), net.status(), e.download_all()))
        e.close()
    (la, sa, ta, A), (lb, sb, tb, W) = got
    assert la.tobytes() == lb.tobytes() and sa.tobytes() == sb.tobytes() and np.array_equal(ta, tb)
    assert same_bits(A, W) and len(la) == 3
    for c in range(3):
        assert sa[c]["n_inactive"] == 60 - masks[c].sum() and sa[c]["n_used"] == la[c]["n"]
        assert sa[c]["n_used"] + sa[c]["n_inactive"] + sa[c]["n_rejected"] == 60
    assert np.array_equal(ta == ref.INACTIVE, masks[2] == 0)
    assert sa["n_rejected"].sum() > 0 and sa["n_used"].min() > 0


# ---- 7. stepping parity ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fuse", [-1, 0])
def test_screened_analysis_then_run_matches_stepper(csim, fuse):
    grid = GRIDS[0]
    nx, ny, dx, dy, loc = grid
    bc = csim.bc_codes("dnpd")
    B = 5
    rng = np.random.default_rng(3)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, _, r = make_network(csim, rng, grid, "point", 20)
    e = csim.Ensemble(B, nx, ny, dx, dy, bc, 0.5)
    e.set_option("fuse", fuse)
    e.upload_all(X)
    e.set_physics(*physics(B))
    e.run(4)
    S = e.download_all()
    hb, vb = obsnet.mv(S, 1, i, j)
    y, mask, _ = screened_values(rng, hb, vb, r)
    net = e.obs_network(i, j, r, loc, log_cycles=1)
    net.set_values(y)
    net.set_active(mask)
    e.assimilate_network(net, inflation=1.05, truth_member=1, record=True, screen=TOL)
    mid = e.download_all()
    assert set(net.status().tolist()) == {0, 1, 2}
    assert not same_bits(mid, S) and exact_bits(mid[1], S[1])
    e.run(7)   # from the ensemble's own buffers: nothing is uploaded again
    got = e.download_all()
    e.close()
    for m in range(B):
        st = csim.Stepper.single(nx, ny, dx, dy, bc, 0.5)
        st.upload(mid[m])
        st.run(*PHYS[m], 7)
        want = st.download()
        st.close()
        assert same_bits(got[m], want), f"member {m}"


# ---- 8. errors ------------------------------------------------------------------------------------------------------------

def code_of(csim, call):
    with pytest.raises(csim.CsimError) as ei:
        call()
    return ei.value.code


def test_errors_leave_everything_as_it_was(csim):
    grid = GRIDS[1]
    nx, ny, dx, dy, loc = grid
    B = 5
    rng = np.random.default_rng(8)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, _, r = make_network(csim, rng, grid, "point", 20)
    e, other = ensemble(csim, X, grid), ensemble(csim, X, grid)
    net = e.obs_network(i, j, r, loc, ordered=True, log_cycles=1)
    foreign = other.obs_network(i, j, r, loc)
    L, C = csim.lib(), csim.C
    buf = (C.c_ubyte * 20)()
    # before any analysis there is no status
    assert code_of(csim, net.status) == 4
    assert L.csim_obs_network_status(net._h, None) == 1
    hb, vb = obsnet.mv(X, None, i, j)
    y, mask, _ = screened_values(rng, hb, vb, r)
    net.set_values(y), foreign.set_values(y)
    net.set_active(mask)
    e.assimilate_network(net, record=True, screen=TOL)
    st, f, log, slog = net.status(), net.fetch(), net.log(), net.screen_log()
    sums = e.checksums()
    assert set(st.tolist()) == {0, 1, 2}

    def unchanged():
        g = net.fetch()
        return (e.checksums() == sums and exact_bits(g.y, y) and exact_bits(g.bg_mean, f.bg_mean)
                and exact_bits(g.post_var, f.post_var) and np.array_equal(net.status(), st)
                and net.log().tobytes() == log.tobytes() and net.screen_log().tobytes() == slog.tobytes())

    bad_mask = mask.copy()
    bad_mask[7] = 2
    calls = [(lambda: e.assimilate_network(net, screen=-1.0), 1), (lambda: e.assimilate_network(net, screen=np.nan), 1),
             (lambda: e.assimilate_network(net, screen=np.inf), 1), (lambda: net.set_active(bad_mask), 1),
             (lambda: e.assimilate_network(foreign, screen=TOL), 1), (lambda: other.assimilate_network(net, screen=TOL), 1),
             (lambda: e.assimilate_network(net, inflation=0.5, screen=TOL), 1),
             (lambda: e.assimilate_network(net, record=2, screen=TOL), 1),
             (lambda: e.assimilate_network(net, record=True, screen=TOL), 4)]          # the log is full
    for k, (call, code) in enumerate(calls):
        assert code_of(csim, call) == code, k
        assert unchanged(), k
    assert L.csim_ensemble_assimilate_screened(e._h, None, 1.0, -1, 0, TOL) == 1
    assert L.csim_ensemble_assimilate_screened(None, net._h, 1.0, -1, 0, TOL) == 1
    assert L.csim_obs_network_screen_log(net._h, 1, None, None) == 1 and L.csim_obs_network_screen_log(net._h, -1, None, None) == 1
    with pytest.raises(ValueError):
        net.set_active(mask[:5])
    assert unchanged() and exact_bits(other.download_all(), X)
    # the refused mask left the old one in place: the same analysis on a twin state uses the same observations
    twin = ensemble(csim, X, grid)
    tnet = twin.obs_network(i, j, r, loc, ordered=True)
    tnet.set_values(y)
    tnet.set_active(mask)
    twin.assimilate_network(tnet, screen=TOL)
    assert twin.checksums() == sums
    twin.assimilate_network(tnet, screen=TOL)
    e.assimilate_network(net, screen=TOL)
    assert twin.checksums() == e.checksums() and np.array_equal(tnet.status(), net.status())
    # set_reports: NaN is a missing report; set_values keeps refusing it
    rep = y.copy()
    rep[[2, 5]] = np.nan
    assert code_of(csim, lambda: net.set_values(rep)) == 1
    net.set_reports(rep)
    e.assimilate_network(net)
    got = net.status()
    assert got[2] == got[5] == ref.INACTIVE and np.count_nonzero(got) == 2
    assert exact_bits(net.fetch().y, np.where(np.isnan(rep), 0.0, rep))
    e.close(), other.close(), twin.close()


# ---- 9. what it is for ---------------------------------------------------------------------------------------------------

OSSE = dict(grid=GRIDS[1], B=13, cycles=3, seed=2, share=0.05, size=3.0, tol=4.0, r=0.01)


def osse_setup():
    """a smooth truth (member 0), twelve members around another smooth field, 112 stations on a 2 x 2 lattice"""
    nx, ny, dx, dy, loc = OSSE["grid"]
    rng = np.random.default_rng(OSSE["seed"])
    jj, ii = np.meshgrid(np.arange(ny + 2), np.arange(nx + 2), indexing="ij")

    def smooth():
        a = rng.standard_normal(4)
        return (a[0] * np.sin(2 * np.pi * ii / nx) + a[1] * np.cos(2 * np.pi * jj / ny)
                + a[2] * np.sin(2 * np.pi * (ii / nx + jj / ny)) + a[3] * np.cos(4 * np.pi * ii / nx)) / 2.0

    X = np.empty((OSSE["B"], ny + 2, nx + 2))
    X[0] = smooth()
    base = X[0] + 0.3 * smooth()
    for m in range(1, OSSE["B"]):
        X[m] = base + 0.3 * smooth() + 0.02 * rng.standard_normal((ny + 2, nx + 2))
    I, J = np.meshgrid(np.arange(2, nx, 2), np.arange(2, ny, 2))
    i, j = I.ravel().astype(np.int32), J.ravel().astype(np.int32)
    reports = []
    for cyc in range(OSSE["cycles"]):
        y = X[0][j, i] + np.sqrt(OSSE["r"]) * rng.standard_normal(len(i))
        bad = rng.permutation(len(i))[:max(1, int(round(OSSE["share"] * len(i))))]
        y[bad] += OSSE["size"] * np.where(rng.uniform(size=len(bad)) < 0.5, -1.0, 1.0)
        reports.append((y, bad))
    return X, i, j, reports


def rmse_of_mean(X):
    return float(np.sqrt(np.mean((X[1:, 1:-1, 1:-1].mean(axis=0) - X[0, 1:-1, 1:-1]) ** 2)))


def osse_restated(csim, screen):
    """the scenario through the numpy restatement alone: the final state and the statuses of every cycle"""
    nx, ny, dx, dy, loc = OSSE["grid"]
    X, i, j, reports = osse_setup()
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    lev = csim.ensemble_assim_plan(i, j, rho.shape[1] // 2, rho.shape[0] // 2, False)
    sts = []
    for y, _ in reports:
        hb, vb = obsnet.mv(X, 0, i, j)
        st = ref.statuses(y, hb, vb, OSSE["r"], screen, None)
        X = ref.subset_analysis(X, rho, lev, i, j, ref.point_taps(len(i)), y, OSSE["r"], 1.0, 0, st)
        sts.append(st)
    return X, sts


def test_osse_screening_keeps_corrupted_reports_out(csim):
    """Three analyses of a static state with 5 % of the reports corrupted by +-3 (thirty standard deviations of the
    observation error), from the same seeds with and without screen = 4: every corrupted report is REJECTED, and the
    RMSE of the forecast mean against the truth member at the end is lower with screening.  Both are comparisons.  The
    same scenario was run through the numpy restatement on the CPU (osse_restated above) before this test was written,
    and seed and corruption size were kept because both statements hold there; the test runs it again and also asserts
    that the GPU gives the restatement's bits."""
    nx, ny, dx, dy, loc = OSSE["grid"]
    X, i, j, reports = osse_setup()
    final = {}
    for screen in (OSSE["tol"], None):
        e = ensemble(csim, X, OSSE["grid"])
        net = e.obs_network(i, j, OSSE["r"], loc, log_cycles=OSSE["cycles"])
        for y, bad in reports:
            net.set_values(y)
            e.assimilate_network(net, truth_member=0, record=True, screen=screen)
            if screen:
                st = net.status()
                assert (st[bad] == ref.REJECTED).all()
        final[screen] = e.download_all()
        if screen:
            slog = net.screen_log()
            assert (slog["n_rejected"] >= len(reports[0][1])).all() and (slog["n_inactive"] == 0).all()
        e.close()
        want, sts = osse_restated(csim, screen or 0.0)
        assert same_bits(final[screen], want)
    with_s, without = rmse_of_mean(final[OSSE["tol"]]), rmse_of_mean(final[None])
    print(f"rmse of the mean against the truth: {rmse_of_mean(X):.5f} at the start, {with_s:.5f} with screening, "
          f"{without:.5f} without")
    assert with_s < without
