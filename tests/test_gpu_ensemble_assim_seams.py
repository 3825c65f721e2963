"""The EnSRF analysis (k_assim_prior, k_assim_update behind csim_ensemble_assimilate, csim_ensemble_assimilate_network
and the screened form) at its launch seams, bit for bit against numpy restatements of the csim.h block:
  A. a level cut into two batches (M = 1024: 8192 observations per batch, level 0 has 9000), where h'_k is indexed
     within the batch and everything else by plan position;
  B. more than 65535 observations in one launch, where the update's grid wraps and a block handles two observations
     in turn;
  C. every register step of the update (P = 4 .. 64) with M = P and M = P + 1 against the per-observation restatement;
  D. a window that covers the whole grid, with lanes of its only wave past its end, then the impact of the same
     analysis (tests/impact_restatement.py): the update and the impact take the same cells of the same windows.
A and B use the level-vectorised restatement of tests/assim_level_restatement.py, which
tests/test_assim_level_restatement_host.py pins to the per-observation ones and which also pins the preconditions of the
cases here (half-widths, level sizes) from the planner alone.  No tolerance anywhere."""
import numpy as np
import pytest

import assim_level_restatement as lvl
import impact_restatement as imp
import obsnet_restatement as obsnet
import screen_restatement as screen
from __graft_entry__ import load_package
from test_gpu_ensemble_assim import make_obs, restate, same_bits

pytestmark = pytest.mark.gpu

TOL = 4.0


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def exact_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def log_matches(row, rec, fields):
    return all(exact_bits(row[f], rec[f]) for f in fields)


def assert_members(G, W, X, t):
    """all members with their ghost rings against the restatement; the ring and the truth member keep the input's bits"""
    for m in range(X.shape[0]):
        assert same_bits(G[m], W[m]), f"member {m} differs from the restatement"
    ring = np.ones(X.shape[1:], dtype=bool)
    ring[1:-1, 1:-1] = False
    assert exact_bits(G[:, ring], X[:, ring]), "ghost ring"
    if t is not None:
        assert exact_bits(G[t], X[t]), "truth member"


# ---- the cases (tests/test_assim_level_restatement_host.py pins their preconditions) -------------------------------

A_GRID = dict(nx=100, ny=90, dx=1.0, dy=1.0, loc=0.4)      # lx = ly = 0: a 1 x 1 table of 1.0
A_MEMBERS = 1024                                           # batches of 2^23 / 1024 = 8192 observations
B_GRID = dict(dx=1.0, dy=1.0, loc=0.6)                     # lx = ly = 1: 3 x 3 windows, +0 in their corners
B_MEMBERS = 5
GRID_Y = 65535                                             # ASSIM_GRID_Y of ensemble_assim.hip


def case_a_obs():
    """every one of the 9000 cells once in shuffled order, 50 of them a second and 5 of those a third time: levels of
    9000, 50 and 5 observations.  The repeats are strewn among the first observations that come after their cell's own,
    so plan order is not input order; 45 of the repeated cells have their first observation in the first batch of
    level 0 and 5 in the second (of the 5 seen three times, 4 and 1)"""
    rng = np.random.default_rng(8192)
    nx, ny = A_GRID["nx"], A_GRID["ny"]
    n, batch = nx * ny, 2**23 // A_MEMBERS
    cells = rng.permutation(n)            # entry k: the cell whose first observation is at position k of level 0
    again = np.concatenate([rng.choice(batch, 45, replace=False), batch + rng.choice(n - batch, 5, replace=False)])
    third = again[[0, 1, 2, 3, 49]]
    # input order by a key: the first observations keep k, a repeat comes somewhere between its cell's k and the end
    key = np.concatenate([np.arange(float(n)), again + rng.uniform(0.1, 0.5, 50) * (n - again),
                          third + rng.uniform(0.6, 0.9, 5) * (n - third)])
    c = np.concatenate([cells, cells[again], cells[third]])[np.argsort(key, kind="stable")]
    return (c % nx + 1).astype(np.int32), (c // nx + 1).astype(np.int32)


def case_b_obs(n):
    """the lattice {2, 5, ..} squared on an n x n grid (n = 780: 260^2 = 67 600, n = 768: 256^2 = 65 536), whose 3 x 3
    windows tile the grid; for n = 780 also 40 of those cells a second time (level 1); all shuffled"""
    rng = np.random.default_rng(n)
    g = np.arange(2, n + 1, 3)
    I, J = np.meshgrid(g, g)
    i, j = I.ravel(), J.ravel()
    if n == 780:
        again = rng.choice(len(i), 40, replace=False)
        i, j = np.concatenate([i, i[again]]), np.concatenate([j, j[again]])
    p = rng.permutation(len(i))
    return i[p].astype(np.int32), j[p].astype(np.int32)


def positions(csim, i, j, lx, ly, ordered):
    """(order, pos): the observation at each plan position, and the plan position of each observation"""
    order = lvl.plan_order(csim.ensemble_assim_plan(i, j, lx, ly, ordered))
    pos = np.empty(len(order), dtype=np.intp)
    pos[order] = np.arange(len(order))
    return order, pos


def screened_values(rng, hb, vb, r, mask, bad):
    """values half a standard deviation of the innovation from the background, those of `bad` 50 away; inactive ones
    hold garbage that must never be looked at"""
    sd = np.sqrt(vb + r)
    y = hb + 0.5 * sd * rng.standard_normal(len(hb)).clip(-2, 2)
    y[bad] = hb[bad] + 50.0 * sd[bad] * np.where(np.arange(len(bad)) % 2, -1.0, 1.0)
    given = y.copy()
    given[mask == 0] = 1e30
    return y, given


# ---- A. two batches in one level ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def case_a():
    g = A_GRID
    i, j = case_a_obs()
    rng = np.random.default_rng(1024)
    X = rng.standard_normal((A_MEMBERS + 1, g["ny"] + 2, g["nx"] + 2))
    X.setflags(write=False)
    r = rng.uniform(0.05, 2.0, len(i))
    return dict(X=X, i=i, j=j, r=r)


def members_a(case, with_truth):
    """(X, t): B = 1025 with truth member 512, or B = 1024 without"""
    return (case["X"], 512) if with_truth else (case["X"][:A_MEMBERS], None)


def ensemble_a(csim, X):
    g = A_GRID
    e = csim.Ensemble(X.shape[0], g["nx"], g["ny"], g["dx"], g["dy"], (0, 1, 2, 0))
    e.upload_all(X)
    return e


def level_a(csim, X, i, j, y, r, lam, t, ordered, **kw):
    g = A_GRID
    return lvl.analysis(csim, X, g["dx"], g["dy"], i, j, y, r, g["loc"], lam, t, ordered, **kw)


@pytest.mark.parametrize("with_truth,lam,ordered", [(True, 1.0, False), (False, 1.05, False), (True, 1.05, True),
                                                    (False, 1.0, True)])
def test_two_batches_assimilate(csim, case_a, with_truth, lam, ordered):
    X, t = members_a(case_a, with_truth)
    i, j, r = case_a["i"], case_a["j"], case_a["r"]
    y = np.random.default_rng(11).standard_normal(len(i))
    e = ensemble_a(csim, X)
    got = e.assimilate(i, j, y, r, A_GRID["loc"], inflation=lam, truth_member=t, ordered=ordered)
    G = e.download_all()
    e.close()
    W, pm, pv, nl = level_a(csim, X, i, j, y, r, lam, t, ordered)
    assert got.nlevels == nl == 3
    assert_members(G, W, X, t)
    qm, qv = lvl.mv(W, t, i, j)
    for name, a, b in (("prior_mean", got.prior_mean, pm), ("prior_var", got.prior_var, pv),
                       ("post_mean", got.post_mean, qm), ("post_var", got.post_var, qv)):
        assert same_bits(a, b), name


def test_two_batches_network_two_cycles(csim, case_a):
    """a point network: the batches are made at the first analysis and reused, with the buffers, by the second"""
    X, t = members_a(case_a, False)
    i, j, r = case_a["i"], case_a["j"], case_a["r"]
    lam, rng = 1.05, np.random.default_rng(12)
    e = ensemble_a(csim, X)
    net = e.obs_network(i, j, r, A_GRID["loc"], log_cycles=2)
    assert net.info == (len(i), 3, 0, 0)
    before, want = X, []
    for cycle in range(2):
        y = rng.standard_normal(len(i))
        net.set_values(y)
        e.assimilate_network(net, inflation=lam, truth_member=t, record=True)
        G = e.download_all()
        W = level_a(csim, before, i, j, y, r, lam, t, False)[0]
        assert_members(G, W, before, t)
        f = net.fetch()
        hb, vb = lvl.mv(before, t, i, j)
        ha, va = lvl.mv(W, t, i, j)
        for name, a, b in (("bg_mean", f.bg_mean, hb), ("bg_var", f.bg_var, vb), ("post_mean", f.post_mean, ha),
                           ("post_var", f.post_var, va)):
            assert same_bits(a, b), f"cycle {cycle}: {name}"
        want.append(obsnet.cycle(y, hb, vb, ha, va, r))
        assert not net.status().any()
        before = W
    log = net.log()
    assert len(log) == 2
    for c in range(2):
        assert log_matches(log[c], want[c], obsnet.FIELDS), f"log record {c}"
    e.close()


def test_two_batches_screened(csim, case_a):
    """a third of the observations masked out and a handful rejected, on both sides of plan position 8192"""
    X, t = members_a(case_a, True)
    i, j, r = case_a["i"], case_a["j"], case_a["r"]
    lam, ordered, n = 1.05, True, len(i)
    batch = 2**23 // A_MEMBERS
    rng = np.random.default_rng(13)
    order, pos = positions(csim, i, j, 0, 0, ordered)
    mask = (rng.uniform(size=n) >= 1.0 / 3.0).astype(np.uint8)
    bad = order[[5, batch - 1, batch, 8999, 9003, n - 1]]      # rejected: both batches of level 0, levels 1 and 2
    mask[bad] = 1
    mask[order[[0, batch - 2, batch + 1, 9001]]] = 0           # inactive at the seam as well
    hb, vb = lvl.mv(X, t, i, j)
    y, given = screened_values(rng, hb, vb, r, mask, bad)
    want_st = screen.statuses(y, hb, vb, r, TOL, mask)
    for st in (screen.INACTIVE, screen.REJECTED):
        at = pos[want_st == st]
        assert (at < batch).any() and ((at >= batch) & (at < 9000)).any() and (at >= 9000).any(), st
    assert np.array_equal(np.flatnonzero(want_st == screen.REJECTED), np.sort(bad))
    e = ensemble_a(csim, X)
    net = e.obs_network(i, j, r, A_GRID["loc"], ordered=ordered, log_cycles=1)
    net.set_values(given)
    net.set_active(mask)
    e.assimilate_network(net, inflation=lam, truth_member=t, record=True, screen=TOL)
    G, st, f = e.download_all(), net.status(), net.fetch()
    assert same_bits(f.bg_mean, hb) and same_bits(f.bg_var, vb)
    assert np.array_equal(st, screen.statuses(given, f.bg_mean, f.bg_var, r, TOL, mask)) and np.array_equal(st, want_st)
    W = level_a(csim, X, i, j, y, r, lam, t, ordered, used=st == screen.USED)[0]
    assert_members(G, W, X, t)
    ha, va = lvl.mv(W, t, i, j)
    assert same_bits(f.post_mean, ha) and same_bits(f.post_var, va)
    counts = (float(np.count_nonzero((mask == 1) & (want_st == screen.USED))), float(np.count_nonzero(mask == 0)),
              float(len(bad)))
    assert net.screen_log().tolist() == [counts]
    assert log_matches(net.log()[0], screen.cycle(given, hb, vb, ha, va, r, st), obsnet.FIELDS)
    e.close()


def linear_taps_at_the_anchor(rng, n):
    """1 to 3 taps per observation, all on the anchor (lx = ly = 0 allows no other), weights of mixed sign"""
    nt = 1 + np.arange(n) % 3
    start = np.concatenate(([0], np.cumsum(nt))).astype(np.int32)
    w = rng.uniform(0.25, 1.0, start[-1]) * np.where(rng.uniform(size=start[-1]) < 0.3, -1.0, 1.0)
    w[start[:-1]] = np.abs(w[start[:-1]])
    return start, np.zeros(start[-1], dtype=np.int32), np.zeros(start[-1], dtype=np.int32), w


def test_two_batches_linear_network(csim, case_a):
    """linear observations: tstart[q] and `first` cross the seam in k_assim_prior<true>"""
    X, t = members_a(case_a, True)
    i, j, r = case_a["i"], case_a["j"], case_a["r"]
    lam, n = 1.05, len(i)
    rng = np.random.default_rng(14)
    taps = linear_taps_at_the_anchor(rng, n)
    y = rng.standard_normal(n)
    e = ensemble_a(csim, X)
    net = e.obs_network(i, j, r, A_GRID["loc"], log_cycles=1, taps=taps)
    assert net.info == (n, 3, 0, 0) and net.ntaps == taps[0][-1]
    net.set_values(y)
    e.assimilate_network(net, inflation=lam, truth_member=t, record=True)
    G, f = e.download_all(), net.fetch()
    W = level_a(csim, X, i, j, y, r, lam, t, False, taps=taps)[0]
    assert_members(G, W, X, t)
    hb, vb = lvl.mv(X, t, i, j, taps)
    ha, va = lvl.mv(W, t, i, j, taps)
    for name, a, b in (("bg_mean", f.bg_mean, hb), ("bg_var", f.bg_var, vb), ("post_mean", f.post_mean, ha),
                       ("post_var", f.post_var, va)):
        assert same_bits(a, b), name
    assert log_matches(net.log()[0], obsnet.cycle(y, hb, vb, ha, va, r), obsnet.FIELDS)
    e.close()


# ---- B. more than 65535 observations in one launch ------------------------------------------------------------------

@pytest.fixture(scope="module")
def case_b():
    i, j = case_b_obs(780)
    rng = np.random.default_rng(780)
    X = rng.standard_normal((B_MEMBERS + 1, 782, 782))
    X.setflags(write=False)
    return dict(X=X, i=i, j=j, r=rng.uniform(0.05, 2.0, len(i)))


def ensemble_b(csim, X):
    n = X.shape[1] - 2
    e = csim.Ensemble(X.shape[0], n, n, B_GRID["dx"], B_GRID["dy"], (0, 1, 2, 0))
    e.upload_all(X)
    return e


def level_b(csim, X, i, j, y, r, lam, t, ordered, **kw):
    g = B_GRID
    return lvl.analysis(csim, X, g["dx"], g["dy"], i, j, y, r, g["loc"], lam, t, ordered, **kw)


def outside_b(csim, shape, i, j):
    """cells that no window writes: the ghost ring and, since the windows tile the grid, their corners (rho = +0)"""
    n = shape[0] - 2
    rho = csim.ensemble_gc_table(B_GRID["dx"], B_GRID["dy"], B_GRID["loc"], n, n)
    out = np.ones(shape, dtype=bool)
    for b in (-1, 0, 1):
        for a in (-1, 0, 1):
            if rho[b + 1, a + 1] > 0:
                out[j + b, i + a] = False
    out[0, :] = out[-1, :] = out[:, 0] = out[:, -1] = True
    return out


@pytest.mark.parametrize("lam,ordered", [(1.0, False), (1.05, True)])
def test_wrapped_grid_assimilate(csim, case_b, lam, ordered):
    X, i, j, r, t = case_b["X"], case_b["i"], case_b["j"], case_b["r"], 2
    y = np.random.default_rng(21).standard_normal(len(i))
    e = ensemble_b(csim, X)
    got = e.assimilate(i, j, y, r, B_GRID["loc"], inflation=lam, truth_member=t, ordered=ordered)
    G = e.download_all()
    e.close()
    W, pm, pv, nl = level_b(csim, X, i, j, y, r, lam, t, ordered)
    assert got.nlevels == nl == 2
    assert_members(G, W, X, t)
    qm, qv = lvl.mv(W, t, i, j)
    for name, a, b in (("prior_mean", got.prior_mean, pm), ("prior_var", got.prior_var, pv),
                       ("post_mean", got.post_mean, qm), ("post_var", got.post_var, qv)):
        assert same_bits(a, b), name
    if lam == 1.0:
        out = outside_b(csim, X.shape[1:], i, j)
        assert np.count_nonzero(~out) == 5 * 260 * 260
        assert exact_bits(G[:, out], X[:, out]), "cells outside every window"


def test_exactly_one_wrapped_observation(csim):
    """65 536 observations: the block of observation 0 is the only one that goes round again"""
    i, j = case_b_obs(768)
    rng = np.random.default_rng(768)
    X = rng.standard_normal((B_MEMBERS + 1, 770, 770))
    y, r, t = rng.standard_normal(len(i)), rng.uniform(0.05, 2.0, len(i)), 2
    e = ensemble_b(csim, X)
    assert e.assimilate(i, j, y, r, B_GRID["loc"], truth_member=t, diagnostics=False) == 1
    G = e.download_all()
    e.close()
    W = level_b(csim, X, i, j, y, r, 1.0, t, False)[0]
    assert_members(G, W, X, t)


def test_wrapped_grid_screened(csim, case_b):
    """a block of the update handles plan positions q and q + 65535 of level 0 in turn (q < 67 600 - 65535 = 2065):
    the first of the two skipped, the second, and both, once by the mask and once by the background check"""
    X, i, j, r, t = case_b["X"], case_b["i"], case_b["j"], case_b["r"], 2
    lam, n, wrapped = 1.05, len(i), 67600 - GRID_Y
    rng = np.random.default_rng(22)
    order, pos = positions(csim, i, j, 1, 1, False)
    mask = (rng.uniform(size=n) >= 0.1).astype(np.uint8)
    pairs = np.array([7, 100, wrapped - 1, 11, 300, 1000])
    mask[order[pairs]] = mask[order[pairs + GRID_Y]] = 1
    off_q = [7, 100 + GRID_Y, wrapped - 1, wrapped - 1 + GRID_Y, 67600 + 3]       # first, second, both; level 1
    bad_q = [11, 300 + GRID_Y, 1000, 1000 + GRID_Y, 67600 + 5]
    mask[order[off_q]] = 0
    mask[order[bad_q]] = 1
    bad = order[bad_q]
    hb, vb = lvl.mv(X, t, i, j)
    y, given = screened_values(rng, hb, vb, r, mask, bad)
    want_st = screen.statuses(y, hb, vb, r, TOL, mask)
    by_q = want_st[order]
    U, I, R = screen.USED, screen.INACTIVE, screen.REJECTED
    assert [(by_q[q], by_q[q + GRID_Y]) for q in pairs] == [(I, U), (U, I), (I, I), (R, U), (U, R), (R, R)]
    assert by_q[67600 + 3] == I and by_q[67600 + 5] == R and np.count_nonzero(by_q == R) == len(bad_q)
    e = ensemble_b(csim, X)
    net = e.obs_network(i, j, r, B_GRID["loc"], log_cycles=1)
    assert net.info == (n, 2, 1, 1)
    net.set_values(given)
    net.set_active(mask)
    e.assimilate_network(net, inflation=lam, truth_member=t, record=True, screen=TOL)
    G, st, f = e.download_all(), net.status(), net.fetch()
    assert same_bits(f.bg_mean, hb) and same_bits(f.bg_var, vb)
    assert np.array_equal(st, screen.statuses(given, f.bg_mean, f.bg_var, r, TOL, mask)) and np.array_equal(st, want_st)
    W = level_b(csim, X, i, j, y, r, lam, t, False, used=st == U)[0]
    assert_members(G, W, X, t)
    ha, va = lvl.mv(W, t, i, j)
    assert same_bits(f.post_mean, ha) and same_bits(f.post_var, va)
    counts = (float(np.count_nonzero(want_st == U)), float(np.count_nonzero(mask == 0)), float(len(bad_q)))
    assert net.screen_log().tolist() == [counts]
    assert log_matches(net.log()[0], screen.cycle(given, hb, vb, ha, va, r, st), obsnet.FIELDS)
    e.close()


# ---- C. every register step against the per-observation restatement -------------------------------------------------

SPACINGS = [(1.0, 1.0), (0.7, 1.3), (1.0, 0.6)]
# M, truth member (none / first / middle / last), inflation, ordered, spacing, nasty values: M = P (no clamped load)
# and M = P + 1 (the next step, mostly clamped) for P = 4, 8, 16, 32, 48; the columns rotate at different strides
STEPS = [(4, None, 1.0, False, 0, True), (5, "first", 1.1, True, 1, False), (8, "middle", 1.1, False, 2, False),
         (9, "last", 1.0, True, 0, True), (16, None, 1.1, True, 1, True), (17, "first", 1.0, False, 2, False),
         (32, "middle", 1.0, True, 0, False), (33, "last", 1.1, False, 1, True), (48, None, 1.1, False, 2, True),
         (49, "first", 1.0, True, 0, False)]


@pytest.mark.parametrize("M,truth,lam,ordered,spacing,nasty", STEPS,
                         ids=[f"M{c[0]}_{c[1]}_lam{c[2]}_ord{int(c[3])}_d{c[4]}_nasty{int(c[5])}" for c in STEPS])
def test_register_steps(csim, M, truth, lam, ordered, spacing, nasty):
    nx, ny, nobs, loc = 37, 29, 40, 2.0
    dx, dy = SPACINGS[spacing]
    B = M if truth is None else M + 1
    t = {None: None, "first": 0, "middle": B // 2, "last": B - 1}[truth]
    rng = np.random.default_rng(100 * M + spacing)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    if nasty:  # as tests/test_gpu_ensemble_assim.py
        X[1, 1, 1] = np.nan
        X[2, ny, nx] = 1e300
        X[:, 2 % ny + 1, 1] = 0.0
        X[0, 2 % ny + 1, 1] = -0.0
        X[3, (ny + 1) // 2, (nx + 1) // 2] = -1e300
    i, j, y, r = make_obs(rng, nx, ny, nobs)
    e = csim.Ensemble(B, nx, ny, dx, dy, (0, 1, 2, 0))
    e.upload_all(X)
    got = e.assimilate(i, j, y, r, loc, inflation=lam, truth_member=t, ordered=ordered)
    G = e.download_all()
    e.close()
    W, pm, pv, qm, qv, nl = restate(csim, X, dx, dy, i, j, y, r, loc, lam, -1 if t is None else t, ordered)
    assert got.nlevels == nl
    assert_members(G, W, X, t)
    for name, a, b in (("prior_mean", got.prior_mean, pm), ("prior_var", got.prior_var, pv),
                       ("post_mean", got.post_mean, qm), ("post_var", got.post_var, qv)):
        assert same_bits(a, b), name


# ---- D. a window over the whole grid, and the impact of the same analysis --------------------------------------------

D_GRID = dict(nx=9, ny=5, dx=1.0, dy=2.0, loc=2.25)        # support 4.5: lx = 4 (4 < 4.5), ly = 2 (2 * 2.0 < 4.5)
D_OBS = [(1, 1), (1, 3), (5, 3)]                           # a corner, the left edge, the middle
D_CELLS = [15, 25, 45]                                     # their windows; 45 = the grid: 19 lanes lie past its end


@pytest.mark.parametrize("M,truth", [(4, None), (5, "last")], ids=["M4_P4_full", "M5_P8_first"])
def test_window_covers_the_grid(csim, M, truth):
    nx, ny, dx, dy, loc = (D_GRID[k] for k in ("nx", "ny", "dx", "dy", "loc"))
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    assert rho.shape == (5, 9)                             # half-widths (4, 2): the full window is the grid
    i, j = (np.array(v, dtype=np.int32) for v in zip(*D_OBS))
    cells = [(min(nx, a + 4) - max(1, a - 4) + 1) * (min(ny, b + 2) - max(1, b - 2) + 1) for a, b in D_OBS]
    assert cells == D_CELLS and nx * ny == 45
    B = M if truth is None else M + 1
    t = None if truth is None else B - 1
    rng = np.random.default_rng(900 + M)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    y, r = rng.standard_normal(3), rng.uniform(0.05, 2.0, 3)
    e = csim.Ensemble(B, nx, ny, dx, dy, (0, 0, 0, 0))
    e.upload_all(X)
    net = e.obs_network(i, j, r, loc, log_cycles=1)
    net.set_values(y)
    e.assimilate_network(net, truth_member=t, record=True)
    net.impact_capture(truth_member=t)
    G = e.download_all()
    W, _, _, _, _, nl = restate(csim, X, dx, dy, i, j, y, r, loc, 1.0, -1 if t is None else t, False)
    assert (net.info.lx, net.info.ly) == (4, 2)
    assert net.info.nlevels == nl == 3                     # every window holds the middle cell: one level each
    assert_members(G, W, X, t)
    w = np.full((ny + 2, nx + 2), np.nan)                  # only the interior is read
    w[1:-1, 1:-1] = rng.standard_normal((ny, nx))
    got = e.obs_impact(net, w)
    e.close()
    hb, _ = obsnet.mv(X, t, i, j)                          # the recorded background: before any observation
    cap = imp.capture(G, t, i, j, None, y, hb, r)
    J = imp.impact(G, cap, rho, i, j, w)
    assert np.count_nonzero(J) == 3 and exact_bits(got.impact, J)
    assert exact_bits(got.summary.total, imp.summary(J, cap.status)[2])
