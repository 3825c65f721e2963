"""The level-vectorised restatement of the analysis (tests/assim_level_restatement.py) on the CPU: bit for bit against
the two per-observation restatements on small grids (`restate` of tests/test_gpu_ensemble_assim.py for point
observations, obsop_restatement.analysis and screen_restatement.subset_analysis for linear and skipped ones), and the
preconditions of the cases of tests/test_gpu_ensemble_assim_seams.py from the planner and the table alone: the
half-widths, the sizes of the levels, the number of levels.  No GPU."""
import numpy as np
import pytest

import assim_level_restatement as lvl
import obsop_restatement as obsop
import screen_restatement as screen
import test_gpu_ensemble_assim_seams as seams
from __graft_entry__ import load_package
from test_gpu_ensemble_assim import make_obs, restate, same_bits


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


NX, NY, NOBS = 9, 7, 40
# dx, dy, loc -> (lx, ly)
GEOMETRY = {(0, 0): (1.0, 1.0, 0.4), (1, 1): (1.0, 1.0, 0.6), (1, 0): (1.0, 2.0, 0.6)}


def members(M, with_truth, nasty, seed):
    B = M + 1 if with_truth else M
    t = B // 2 if with_truth else None
    X = np.random.default_rng(seed).standard_normal((B, NY + 2, NX + 2))
    if nasty:
        X[1, 1, 1] = np.nan
        X[0, NY, NX] = 1e300
        X[:, 3, 1] = 0.0
        X[0, 3, 1] = -0.0
        X[1, (NY + 1) // 2, (NX + 1) // 2] = -1e300
    return X, t


def taps_within(rng, i, j, lx, ly):
    """1 to 3 taps per observation inside its window and the interior, weights of mixed sign, a repeated cell"""
    per = []
    for o in range(len(i)):
        nt = 1 + o % 3
        ci = np.clip(i[o] + rng.integers(-lx, lx + 1, nt), 1, NX)
        cj = np.clip(j[o] + rng.integers(-ly, ly + 1, nt), 1, NY)
        if nt == 3:
            ci[2], cj[2] = ci[0], cj[0]
        per.append((list(ci - i[o]), list(cj - j[o]), list(rng.uniform(-1.0, 1.5, nt))))
    taps = obsop.concat(per)
    assert obsop.check(NX, NY, lx, ly, i, j, taps)
    return taps


CASES = [(M, with_truth, lam, ordered, half) for M in (2, 5, 17) for with_truth in (False, True) for lam in (1.0, 1.1)
         for ordered in (False, True) for half in GEOMETRY]


@pytest.mark.parametrize("M,with_truth,lam,ordered,half", CASES,
                         ids=[f"M{c[0]}_t{int(c[1])}_lam{c[2]}_ord{int(c[3])}_l{c[4][0]}{c[4][1]}" for c in CASES])
def test_level_restatement_is_the_serial_one(csim, M, with_truth, lam, ordered, half):
    dx, dy, loc = GEOMETRY[half]
    rho = csim.ensemble_gc_table(dx, dy, loc, NX, NY)
    assert (rho.shape[1] // 2, rho.shape[0] // 2) == half
    seed = 1000 * M + 100 * with_truth + 10 * ordered + half[0] + half[1]
    rng = np.random.default_rng(seed)
    i, j, y, r = make_obs(rng, NX, NY, NOBS)          # corners, edges, duplicated cells
    i[8], j[8] = i[0], j[0]                           # one cell three times: three levels even with 1 x 1 windows
    lev = csim.ensemble_assim_plan(i, j, half[0], half[1], ordered)
    assert lev.max() + 1 >= 3, "the case needs several levels"
    # point observations, nasty values in the members
    X, t = members(M, with_truth, True, seed)
    W, pm, pv, _, _, nl = restate(csim, X, dx, dy, i, j, y, r, loc, lam, -1 if t is None else t, ordered)
    G, hbar, p, nlevels = lvl.analysis(csim, X, dx, dy, i, j, y, r, loc, lam, t, ordered)
    assert nlevels == nl == lev.max() + 1
    assert same_bits(G, W) and same_bits(hbar, pm) and same_bits(p, pv)
    assert not same_bits(G, X)
    # linear observations
    taps = taps_within(rng, i, j, *half)
    W = obsop.analysis(X, rho, lev, i, j, taps, y, r, lam, t)
    G = lvl.analysis(csim, X, dx, dy, i, j, y, r, loc, lam, t, ordered, taps=taps)[0]
    assert same_bits(G, W) and not same_bits(G, X)
    assert all(same_bits(a, b) for a, b in zip(lvl.mv(X, t, i, j, taps), obsop.mv(X, t, i, j, taps)))
    # skipped observations, linear and point (the one-tap form equals the point form where no -0 is in play)
    used = rng.uniform(size=NOBS) < 0.6
    used[:2] = [False, True]
    status = np.where(used, screen.USED, screen.INACTIVE)
    W = screen.subset_analysis(X, rho, lev, i, j, taps, y, r, lam, t, status)
    G, hbar, p, _ = lvl.analysis(csim, X, dx, dy, i, j, y, r, loc, lam, t, ordered, taps=taps, used=used)
    assert same_bits(G, W)
    assert np.isnan(hbar[~used]).all() and np.isnan(p[~used]).all()
    X, t = members(M, with_truth, False, seed)
    W = screen.subset_analysis(X, rho, lev, i, j, screen.point_taps(NOBS), y, r, lam, t, status)
    G = lvl.analysis(csim, X, dx, dy, i, j, y, r, loc, lam, t, ordered, used=used)[0]
    assert same_bits(G, W) and not same_bits(G, X)


def test_wider_windows_are_refused(csim):
    X = np.zeros((3, NY + 2, NX + 2))
    with pytest.raises(AssertionError):
        lvl.analysis(csim, X, 1.0, 1.0, [1], [1], [0.0], [1.0], 2.0, 1.0, None, False)


# ---- what the seam cases rely on --------------------------------------------------------------------------------------

def level_sizes(csim, i, j, half, ordered):
    return np.bincount(csim.ensemble_assim_plan(i, j, half, half, ordered)).tolist()


def test_case_a_has_two_batches_in_level_0(csim):
    g = seams.A_GRID
    rho = csim.ensemble_gc_table(g["dx"], g["dy"], g["loc"], g["nx"], g["ny"])
    assert rho.shape == (1, 1) and rho[0, 0] == 1.0
    i, j = seams.case_a_obs()
    batch = 2**23 // seams.A_MEMBERS
    assert batch == 8192 and len(i) == 9055
    for ordered in (False, True):
        sizes = level_sizes(csim, i, j, 0, ordered)
        assert sizes == [9000, 50, 5] and batch < sizes[0] < 2 * batch
        # cells observed again have their first observation in both batches of level 0; plan order is not input order
        order, pos = seams.positions(csim, i, j, 0, 0, ordered)
        times = np.zeros((g["ny"] + 2, g["nx"] + 2), dtype=int)
        np.add.at(times, (j, i), 1)
        for k in (2, 3):
            at = pos[(times[j, i] == k) & (pos < sizes[0])]
            assert (at < batch).any() and (at >= batch).any(), f"cells observed {k} times"
        assert not np.array_equal(order, np.arange(len(i)))


@pytest.mark.parametrize("n,sizes", [(780, [67600, 40]), (768, [65536])])
def test_case_b_wraps_the_launch_grid(csim, n, sizes):
    g = seams.B_GRID
    rho = csim.ensemble_gc_table(g["dx"], g["dy"], g["loc"], n, n)
    assert rho.shape == (3, 3) and (rho[1, :] > 0).all() and (rho[:, 1] > 0).all()
    assert (rho[::2, ::2] == 0).all() and not np.signbit(rho).any()
    i, j = seams.case_b_obs(n)
    assert 2**23 // seams.B_MEMBERS >= 2**20 >= len(i), "one batch per level"
    for ordered in (False, True):
        got = level_sizes(csim, i, j, 1, ordered)
        assert got == sizes and got[0] > seams.GRID_Y
    assert sizes[0] - seams.GRID_Y == (2065 if n == 780 else 1)
