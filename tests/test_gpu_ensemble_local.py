"""The local analysis on the GPU (csim_ensemble_assimilate_local), bit for bit against the numpy restatement of the
csim.h block (tests/local_analysis_restatement.py, which tests/test_local_analysis_host.py holds against an eigh LETKF):
point and linear networks, a lone observation against the serial filter, a dense network, mask and background check with
both logs, the diagnostics and the forecast impact, every tile and pack of the launch, the limits, and the whole cycle
enqueued with stepping parity.  Everything is compared through integer views; ghost rings and the truth member are part
of every comparison, the other ping-pong buffer through the runs that follow an analysis.  The grids are small: what is
under test goes per cell and per local list, not per grid."""
import numpy as np
import pytest

import impact_restatement as imp
import local_analysis_restatement as ref
import obsnet_restatement as obsnet
import obsop_restatement as obsop
import screen_restatement as screen
import test_gpu_ensemble_obsop as obsop_net
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

# nx, ny, dx, dy, loc: half-widths (4, 4), (4, 4) and, anisotropic, (3, 4); last the grid of the `net40` network
GRIDS = [(37, 21, 1.0, 1.0, 2.5), (16, 16, 1.0, 1.0, 2.5), (37, 21, 1.0, 0.8, 2.0),
         (obsop_net.NX, obsop_net.NY, obsop_net.DX, obsop_net.DY, obsop_net.LOC)]
HALF = [(4, 4), (4, 4), (3, 4), (obsop_net.LX, obsop_net.LY)]
NOBS = 40


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    for grid, (lx, ly) in zip(GRIDS, HALF):
        nx, ny, dx, dy, loc = grid
        tab = pkg.ensemble_gc_table(dx, dy, loc, nx, ny)
        assert (tab.shape[1] // 2, tab.shape[0] // 2) == (lx, ly)
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


def truth_of(where, B):
    return {None: None, "first": 0, "middle": B // 2, "last": B - 1}[where]


def cells_of(rng, grid, nobs):
    """random cells with the four corners, an edge and two observations on one cell"""
    nx, ny = grid[0], grid[1]
    i, j = rng.integers(1, nx + 1, nobs), rng.integers(1, ny + 1, nobs)
    i[:5], j[:5] = [1, nx, 1, nx, (nx + 1) // 2], [1, ny, ny, 1, 1]
    i[6], j[6] = i[5], j[5]
    return i.astype(np.int32), j.astype(np.int32)


def make_network(csim, rng, grid, kind, nobs=NOBS):
    """(i, j, taps or None, r): point observations; bilinear stations between grid points; 3 x 3 footprints clipped at
    the sides; `custom`: hand-made operators with a repeated cell and a negative weight; `net40`: the 40 observations
    of tests/test_gpu_ensemble_obsop.py on their grid, 1, 4, 25 and 64 taps among them"""
    nx, ny = grid[0], grid[1]
    if kind == "net40":
        assert nobs == 40 and grid == GRIDS[3]
        return obsop_net.network()
    r = rng.uniform(0.05, 2.0, nobs)
    if kind == "bilinear":
        x, y = rng.uniform(1, nx, nobs), rng.uniform(1, ny, nobs)
        x[:4], y[:4] = [1.0, nx, 1.25, nx - 0.5], [1.0, ny, ny - 0.25, 1.5]
        i, j, taps = csim.bilinear_taps(nx, ny, x, y)
        return i, j, tuple(taps), r
    i, j = cells_of(rng, grid, nobs)
    if kind == "box":
        i, j, taps = csim.box_taps(nx, ny, i, j, 1, 1)
        return i, j, tuple(taps), r
    if kind == "custom":
        per = []
        for o in range(nobs):
            a = 1 if i[o] < nx else -1
            b = 1 if j[o] < ny else -1
            per.append(([0, a, 0, 0], [0, 0, b, 0], [0.75, -0.5, 0.5, 0.25]))    # the anchor twice, one weight < 0
        return i, j, obsop.concat(per), r
    return i, j, None, r


def check_untouched(A, X, grid, rho, i, j, r, t, status=None):
    """ghost rings, the truth member and the cells outside every support keep their bits"""
    ring = np.ones(X.shape[1:], dtype=bool)
    ring[1:-1, 1:-1] = False
    assert exact_bits(A[:, ring], X[:, ring])
    if t is not None:
        assert exact_bits(A[t], X[t])
    far = ~ref.touched(X.shape[1:], rho, i, j, r, status) & ~ring
    return far


# ---- 1. bits ---------------------------------------------------------------------------------------------------------

# every M of the list with both grids and the anisotropic table between them; the truth member first, in the middle,
# last and nowhere; inflation 1 and 1.1; Dirichlet, Neumann and mixed sides
BITS = [(2, "first", 1, 1.0, "dddd"), (2, None, 2, 1.1, "nnnn"), (5, "middle", 0, 1.1, "nnnn"), (5, "last", 1, 1.0, "dnpd"),
        (8, None, 2, 1.1, "dnpd"), (8, "first", 1, 1.0, "nnnn"), (33, "last", 0, 1.0, "dddd"), (33, None, 1, 1.1, "dnpd"),
        (64, None, 1, 1.0, "dddd"), (64, "middle", 2, 1.1, "nddn")]


@pytest.mark.parametrize("case", BITS, ids=[f"M{c[0]}_t{c[1]}_grid{c[2]}_lam{c[3]}_{c[4]}" for c in BITS])
def test_local_analysis_is_the_restatement(csim, case):
    M, where, gi, lam, bcs = case
    grid = GRIDS[gi]
    nx, ny, dx, dy, loc = grid
    B = M if where is None else M + 1
    t = truth_of(where, B)
    rng = np.random.default_rng(100 * M + gi)
    X0 = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, _, r = make_network(csim, rng, grid, "point")
    y = rng.standard_normal(NOBS)
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    e = ensemble(csim, X0, grid, bcs)
    e.run(2)                          # the ghost rings are those of the sides
    X = e.download_all()
    net = e.obs_network(i, j, r, loc)
    _, most = csim.obs_local_count(nx, ny, i, j, *HALF[gi])
    assert net.local_info() == most and 2 <= most <= 64 and most * M <= 4096
    net.set_values(y)
    e.assimilate_local(net, inflation=lam, truth_member=t)
    A = e.download_all()
    want = ref.analysis(X, rho, i, j, None, y, r, lam, t)
    assert same_bits(A, want) and not same_bits(A, X)
    far = check_untouched(A, X, grid, rho, i, j, r, t)
    assert far.any() or gi == 1       # 40 windows of 9 x 9 cover the small grid
    if lam == 1.0:                    # (the inflation alone writes every interior cell)
        assert exact_bits(A[:, far], X[:, far])
    assert not net.status().any()
    e.close()


# ---- 2. linear networks ------------------------------------------------------------------------------------------------

LINEAR = [("bilinear", 5, "middle", 0, 1.1), ("box", 8, None, 1, 1.0), ("custom", 33, "last", 2, 1.1),
          ("box", 65, None, 1, 1.0), ("bilinear", 64, "first", 2, 1.0), ("net40", 65, "last", 3, 1.0)]


@pytest.mark.parametrize("case", LINEAR, ids=[f"{c[0]}_M{c[1]}_t{c[2]}_grid{c[3]}_lam{c[4]}" for c in LINEAR])
def test_linear_networks(csim, case):
    kind, M, where, gi, lam = case
    grid = GRIDS[gi]
    nx, ny, dx, dy, loc = grid
    B = M if where is None else M + 1
    t = truth_of(where, B)
    rng = np.random.default_rng(200 * M + gi)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    nobs = 40 if kind == "net40" else 30      # net40 at M = 65: 64 taps through two tiles of the linear prior
    i, j, taps, r = make_network(csim, rng, grid, kind, nobs)
    if kind == "custom":
        assert (taps[3] < 0).any()
    y = rng.standard_normal(nobs)
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    e = ensemble(csim, X, grid)
    net = e.obs_network(i, j, r, loc, taps=taps, log_cycles=1)
    net.set_values(y)
    e.assimilate_local(net, inflation=lam, truth_member=t, record=True)
    A = e.download_all()
    assert same_bits(A, ref.analysis(X, rho, i, j, taps, y, r, lam, t)) and not same_bits(A, X)
    check_untouched(A, X, grid, rho, i, j, r, t)
    f = net.fetch()
    hb, vb = obsop.mv(X, t, i, j, taps)
    ha, va = obsop.mv(A, t, i, j, taps)
    assert same_bits(f.bg_mean, hb) and same_bits(f.bg_var, vb) and same_bits(f.post_mean, ha) and same_bits(f.post_var, va)
    e.close()


# ---- 3. a lone point observation: the serial filter at the observed cell -------------------------------------------------

@pytest.mark.parametrize("case", [(5, None, 1.0), (33, "middle", 1.1), (65, "last", 1.0)],
                         ids=lambda c: f"M{c[0]}_t{c[1]}_lam{c[2]}")
def test_lone_observation_is_the_serial_filter_at_its_cell(csim, case):
    """there rho = 1 and the two definitions coincide, which pins the formula to the existing filter"""
    M, where, lam = case
    grid = GRIDS[1]
    nx, ny, dx, dy, loc = grid
    B = M if where is None else M + 1
    t = truth_of(where, B)
    rng = np.random.default_rng(300 + M)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, r, y = np.array([7], dtype=np.int32), np.array([9], dtype=np.int32), np.array([0.4]), np.array([0.8])
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    assert rho[4, 4] == 1.0
    a, b = ensemble(csim, X, grid), ensemble(csim, X, grid)
    na, nb = a.obs_network(i, j, r, loc), b.obs_network(i, j, r, loc)
    na.set_values(y), nb.set_values(y)
    a.assimilate_local(na, inflation=lam, truth_member=t)
    b.assimilate_network(nb, inflation=lam, truth_member=t)
    A, W = a.download_all(), b.download_all()
    assert exact_bits(A[:, 9, 7], W[:, 9, 7]) and not exact_bits(A[:, 9, 7], X[:, 9, 7])
    assert same_bits(A, ref.analysis(X, rho, i, j, None, y, r, lam, t))
    assert na.local_info() == 1
    a.close(), b.close()


# ---- 4. a dense network ----------------------------------------------------------------------------------------------------

def test_dense_network(csim):
    """an observation on every second cell of 24 x 24 with 9 x 9 windows: 25 mutually conflicting observations force the
    serial plan into at least 25 levels; the local analysis is one pass and matches the restatement"""
    grid = (24, 24, 1.0, 1.0, 2.5)
    nx, ny, dx, dy, loc = grid
    B, t = 7, 3
    rng = np.random.default_rng(41)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    I, J = np.meshgrid(np.arange(1, nx + 1, 2), np.arange(1, ny + 1, 2))
    i, j = I.ravel().astype(np.int32), J.ravel().astype(np.int32)
    n = len(i)
    r, y = rng.uniform(0.05, 2.0, n), rng.standard_normal(n)
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    e = ensemble(csim, X, grid)
    net = e.obs_network(i, j, r, loc)
    assert n == 144 and net.info.nlevels >= 25
    assert net.local_info() == 25
    net.set_values(y)
    e.assimilate_local(net, inflation=1.05, truth_member=t)
    A = e.download_all()
    assert same_bits(A, ref.analysis(X, rho, i, j, None, y, r, 1.05, t)) and not same_bits(A, X)
    e.close()


# ---- 5. mask and screening ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["point", "box"])
def test_masked_network_is_the_network_of_the_active_subset(csim, kind):
    """the order is the input index, so leaving observations out is the same as never having had them"""
    grid = GRIDS[0]
    nx, ny, dx, dy, loc = grid
    B, t = 9, 4
    rng = np.random.default_rng(51)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, taps, r = make_network(csim, rng, grid, kind)
    y = rng.standard_normal(NOBS)
    mask = (rng.uniform(size=NOBS) < 0.5).astype(np.uint8)
    mask[5], mask[6] = 1, 0                         # one of the two on one cell
    keep = np.flatnonzero(mask)
    a, b = ensemble(csim, X, grid), ensemble(csim, X, grid)
    na = a.obs_network(i, j, r, loc, taps=taps)
    yy = y.copy()
    yy[mask == 0] = 1e30                            # never looked at
    na.set_values(yy)
    na.set_active(mask)
    sub = None if taps is None else obsop.concat([(list(taps[1][taps[0][o]:taps[0][o + 1]]),
                                                   list(taps[2][taps[0][o]:taps[0][o + 1]]),
                                                   list(taps[3][taps[0][o]:taps[0][o + 1]])) for o in keep])
    nb = b.obs_network(i[keep], j[keep], r[keep], loc, taps=sub)
    nb.set_values(y[keep])
    a.assimilate_local(na, inflation=1.1, truth_member=t)
    b.assimilate_local(nb, inflation=1.1, truth_member=t)
    A, W = a.download_all(), b.download_all()
    assert exact_bits(A, W) and not exact_bits(A, X)
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    st = np.where(mask == 1, screen.USED, screen.INACTIVE)
    assert np.array_equal(na.status(), st) and not nb.status().any()
    assert same_bits(A, ref.analysis(X, rho, i, j, taps, y, r, 1.1, t, st))
    a.close(), b.close()


def test_screened_recorded_analysis_and_its_impact(csim):
    """a mask, a planted gross error that screen = 4 rejects, record = 1: statuses, both logs and the diagnostics are
    the restatement's; then impact_capture and obs_impact after a run give what tests/impact_restatement.py gives"""
    grid = GRIDS[0]
    nx, ny, dx, dy, loc = grid
    B, t, tol = 9, 2, 4.0
    rng = np.random.default_rng(52)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, _, r = make_network(csim, rng, grid, "point")
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    e = ensemble(csim, X, grid)
    net = e.obs_network(i, j, r, loc, log_cycles=2)
    hb, vb = obsnet.mv(X, t, i, j)
    y = hb + 0.5 * np.sqrt(vb + r) * rng.standard_normal(NOBS).clip(-2, 2)
    y[8] = hb[8] + 50.0 * np.sqrt(vb[8] + r[8])     # the gross error
    mask = np.ones(NOBS, dtype=np.uint8)
    mask[[3, 12, 20]] = 0
    net.set_values(y)
    net.set_active(mask)
    st = screen.statuses(y, hb, vb, r, tol, mask)
    assert st[8] == screen.REJECTED and set(st.tolist()) == {0, 1, 2}
    e.assimilate_local(net, inflation=1.05, truth_member=t, record=True, screen=tol)
    A = e.download_all()
    assert same_bits(A, ref.analysis(X, rho, i, j, None, y, r, 1.05, t, st)) and not same_bits(A, X)
    check_untouched(A, X, grid, rho, i, j, r, t, st)
    assert np.array_equal(net.status(), st)
    f = net.fetch()
    ha, va = obsnet.mv(A, t, i, j)
    assert exact_bits(f.y, y) and f.truth is None
    assert same_bits(f.bg_mean, hb) and same_bits(f.bg_var, vb) and same_bits(f.post_mean, ha) and same_bits(f.post_var, va)
    log, slog = net.log(), net.screen_log()
    assert len(log) == 1 and len(slog) == 1
    rec, srec = screen.cycle(y, hb, vb, ha, va, r, st), screen.screen_cycle(st)
    assert all(exact_bits(log[0][k], rec[k]) for k in obsnet.FIELDS), (log[0], rec)
    assert all(exact_bits(slog[0][k], srec[k]) for k in screen.SCREEN_FIELDS), (slog[0], srec)
    # the impact of the recorded local analysis
    net.impact_capture(truth_member=t)
    e.run(3)
    Xf = e.download_all()
    w = np.zeros((ny + 2, nx + 2))
    w[1:-1, 1:-1] = rng.standard_normal((ny, nx)) / (nx * ny)
    got = e.obs_impact(net, w)
    cap = imp.capture(A, t, i, j, None, y, hb, r, st)
    J = imp.impact(Xf, cap, rho, i, j, w)
    assert exact_bits(got.impact, J) and np.count_nonzero(J) == np.count_nonzero(st == 0)
    used, beneficial, total = imp.summary(J, st)
    assert (got.summary.used, got.summary.beneficial) == (used, beneficial) and exact_bits(got.summary.total, total)
    # an unrecorded local analysis replaces the status bytes: no capture from it, as after an unrecorded serial one
    e.assimilate_local(net, truth_member=t)
    with pytest.raises(csim.CsimError) as ei:
        net.impact_capture(truth_member=t)
    assert ei.value.code == 4
    # a second record: the log goes on; a third one finds it full
    e.assimilate_local(net, truth_member=t, record=True)
    assert len(net.log()) == 2 and net.screen_log()[1]["n_inactive"] == 3.0
    with pytest.raises(csim.CsimError) as ei:
        e.assimilate_local(net, truth_member=t, record=True)
    assert ei.value.code == 4
    e.close()


# ---- 6. launch seams ------------------------------------------------------------------------------------------------------------

def test_result_depends_on_neither_tile_nor_pack(csim):
    """every local_tile with every local_pack on 37 x 21: tiles cut by the domain edge (37 = 2 x 16 + 5, 21 = 16 + 5),
    last waves of a tile with a partly filled group (64 or 256 cells in groups of 3), one cell per wave, and a pack
    beyond what fits beside max_local observations, which is cut to that"""
    grid = GRIDS[0]
    nx, ny, dx, dy, loc = grid
    B, t = 6, 5
    rng = np.random.default_rng(61)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, _, r = make_network(csim, rng, grid, "point")
    y = rng.standard_normal(NOBS)
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    want = ref.analysis(X, rho, i, j, None, y, r, 1.1, t)
    e = ensemble(csim, X, grid)
    net = e.obs_network(i, j, r, loc)
    net.set_values(y)
    assert e.get_option("local_tile") == 0 and e.get_option("local_pack") == 0
    assert 64 // net.local_info() >= 4          # the automatic pack and the cut of 64 differ from 1 and 3
    for tile in (4, 8, 16, 0):
        for pack in (1, 3, 0, 64):
            e.upload_all(X)
            e.set_option("local_tile", tile)
            e.set_option("local_pack", pack)
            assert e.get_option("local_tile") == tile and e.get_option("local_pack") == pack
            e.assimilate_local(net, inflation=1.1, truth_member=t)
            assert same_bits(e.download_all(), want), (tile, pack)
    for key, bad in (("local_tile", (-1, 1, 2, 5, 12, 32)), ("local_pack", (-1, 65, 1 << 20))):
        for v in bad:
            with pytest.raises(csim.CsimError) as ei:
                e.set_option(key, v)
            assert ei.value.code == 1
    assert e.get_option("local_tile") == 0 and e.get_option("local_pack") == 64
    e.close()


def block_network(rng, n):
    """n observations inside the 5 x 5 block around cell (5, 4) of a 9 x 7 grid: with half-widths 4 every window holds
    that cell, so max_local = n"""
    return rng.integers(3, 8, n).astype(np.int32), rng.integers(2, 7, n).astype(np.int32)


def test_the_limits_run_at_their_edge(csim):
    """max_local = 64 with M = 64: both bounds met with equality, one cell per wave"""
    grid = (9, 7, 1.0, 1.0, 2.5)
    nx, ny, dx, dy, loc = grid
    rng = np.random.default_rng(62)
    X = rng.standard_normal((64, ny + 2, nx + 2))
    i, j = block_network(rng, 64)
    r, y = rng.uniform(0.05, 2.0, 64), rng.standard_normal(64)
    rho = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    e = ensemble(csim, X, grid)
    net = e.obs_network(i, j, r, loc, ordered=True)
    assert net.local_info() == 64
    net.set_values(y)
    e.assimilate_local(net)
    A = e.download_all()
    assert same_bits(A, ref.analysis(X, rho, i, j, None, y, r, 1.0, None)) and not same_bits(A, X)
    e.close()


def test_beyond_the_limits_is_unsupported_and_changes_nothing(csim):
    """max_local = 65; max_local M = 33 x 128 = 4224 > 4096; nobs M = 262145 x 256 > 2^26: CSIM_ERR_UNSUPPORTED, the
    checksums as before, no status, and the serial analysis still takes the network"""
    grid = (9, 7, 1.0, 1.0, 2.5)
    nx, ny, dx, dy, loc = grid
    rng = np.random.default_rng(63)
    for B, n in ((3, 65), (128, 33)):
        X = rng.standard_normal((B, ny + 2, nx + 2))
        i, j = block_network(rng, n)
        e = ensemble(csim, X, grid)
        net = e.obs_network(i, j, np.full(n, 0.5), loc, ordered=True, log_cycles=1)
        assert net.local_info() == n
        net.set_values(rng.standard_normal(n))
        sums = e.checksums()
        for record in (False, True):
            with pytest.raises(csim.CsimError) as ei:
                e.assimilate_local(net, inflation=1.1, record=record)
            assert ei.value.code == 5 and e.checksums() == sums
        with pytest.raises(csim.CsimError) as ei:
            net.status()
        assert ei.value.code == 4 and len(net.log()) == 0
        # the other errors come first, as in the serial analysis
        with pytest.raises(csim.CsimError) as ei:
            e.assimilate_local(net, inflation=0.5)
        assert ei.value.code == 1
        e.close()
    # the priors of all observations: windows of one cell (loc 0.4), thirteen observations on a cell at most
    grid = (160, 128, 1.0, 1.0, 0.4)
    nx, ny, dx, dy, loc = grid
    B, n = 256, (1 << 26) // 256 + 1
    X = np.zeros((B, ny + 2, nx + 2))
    X[:, 1:-1, 1:-1] = rng.standard_normal((B, 1, nx))
    o = np.arange(n)
    i, j = (o % nx + 1).astype(np.int32), (o // nx % ny + 1).astype(np.int32)
    e = ensemble(csim, X, grid)
    net = e.obs_network(i, j, np.full(n, 0.5), loc, ordered=True)
    assert net.local_info() == 13 and net.info.lx == 0 and net.info.ly == 0
    net.set_values(np.zeros(n))
    sums = e.checksums()
    with pytest.raises(csim.CsimError) as ei:
        e.assimilate_local(net)
    assert ei.value.code == 5 and e.checksums() == sums
    e.close()


def test_errors_are_those_of_the_screened_analysis(csim):
    grid = GRIDS[1]
    nx, ny, dx, dy, loc = grid
    rng = np.random.default_rng(64)
    X = rng.standard_normal((5, ny + 2, nx + 2))
    i, j, _, r = make_network(csim, rng, grid, "point", 20)
    e, other = ensemble(csim, X, grid), ensemble(csim, X, grid)
    net, foreign = e.obs_network(i, j, r, loc), other.obs_network(i, j, r, loc)
    L = csim.lib()

    def code_of(call):
        with pytest.raises(csim.CsimError) as ei:
            call()
        return ei.value.code

    assert code_of(lambda: e.assimilate_local(net)) == 4                       # no values yet
    net.set_values(rng.standard_normal(20)), foreign.set_values(rng.standard_normal(20))
    sums = e.checksums()
    calls = [(lambda: e.assimilate_local(net, screen=-1.0), 1), (lambda: e.assimilate_local(net, screen=np.nan), 1),
             (lambda: e.assimilate_local(foreign), 1), (lambda: other.assimilate_local(net), 1),
             (lambda: e.assimilate_local(net, inflation=0.5), 1), (lambda: e.assimilate_local(net, inflation=np.inf), 1),
             (lambda: e.assimilate_local(net, truth_member=5), 1), (lambda: e.assimilate_local(net, truth_member=-2), 1),
             (lambda: e.assimilate_local(net, record=2), 1), (lambda: e.assimilate_local(net, record=True), 4)]  # no log
    for k, (call, code) in enumerate(calls):
        assert code_of(call) == code, k
        assert e.checksums() == sums, k
    assert L.csim_ensemble_assimilate_local(e._h, None, 1.0, -1, 0, 0.0) == 1
    assert L.csim_ensemble_assimilate_local(None, net._h, 1.0, -1, 0, 0.0) == 1
    assert L.csim_obs_network_local_info(None, None) == 1 and L.csim_obs_network_local_info(net._h, None) == 1
    assert code_of(net.status) == 4                                               # none of them analysed anything
    two = ensemble(csim, X[:2], grid)
    n2 = two.obs_network(i, j, r, loc)
    n2.set_values(np.zeros(20))
    assert code_of(lambda: two.assimilate_local(n2, truth_member=0)) == 1         # one forecast member
    e.close(), other.close(), two.close()


# ---- 7. the cycle ------------------------------------------------------------------------------------------------------------------

def test_whole_local_cycle_enqueued(csim):
    """three cycles of run -> observe -> prior_capture -> assimilate_local(record) -> relax -> perturb with no
    synchronising call in between, then one log: the same as with a sync after every call"""
    grid = GRIDS[0]
    nx, ny, dx, dy, loc = grid
    B, seed = 9, 77
    rng = np.random.default_rng(71)
    X = 0.2 * rng.standard_normal((B, ny + 2, nx + 2))
    X[0] += 1.0
    i, j, _, r = make_network(csim, rng, grid, "point", 60)
    got = []
    for form in ("enqueued", "synced"):
        e = ensemble(csim, X, grid, "dnpd")
        net = e.obs_network(i, j, r, loc, log_cycles=3)
        for cyc in range(3):
            steps = [lambda: e.run(3), lambda: net.observe(0, seed, cyc),
                     lambda: e.prior_capture("spread", truth_member=0),
                     lambda: e.assimilate_local(net, truth_member=0, record=True, screen=1.0),
                     lambda: e.relax(0.6, truth_member=0),
                     lambda: e.perturb(0.05, 3.0, seed, cyc, centered=True, truth_member=0)]
            for step in steps:
                step()
                if form == "synced":
                    e.sync()
        e.run(2)
        got.append((net.log(), net.screen_log(), net.status(), e.download_all()))
        e.close()
    (la, sa, ta, A), (lb, sb, tb, W) = got
    assert la.tobytes() == lb.tobytes() and sa.tobytes() == sb.tobytes() and np.array_equal(ta, tb)
    assert same_bits(A, W) and len(la) == 3 and la["has_truth"].all()
    assert sa["n_rejected"].sum() > 0 and sa["n_used"].min() > 0


@pytest.mark.parametrize("fuse", [-1, 0])
def test_local_analysis_then_run_matches_stepper(csim, fuse):
    """the run after the analysis reads what it wrote and nothing stale from the other buffer: each member equals a
    single Stepper started from the downloaded analysed member; a stats_begin issued before the analysis sees the
    state before it"""
    grid = GRIDS[0]
    nx, ny, dx, dy, loc = grid
    bc = csim.bc_codes("dnpd")
    B = 5
    rng = np.random.default_rng(72)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, _, r = make_network(csim, rng, grid, "point", 20)
    e = csim.Ensemble(B, nx, ny, dx, dy, bc, 0.5)
    e.set_option("fuse", fuse)
    e.upload_all(X)
    e.set_physics(*physics(B))
    e.run(4)
    S = e.download_all()
    before = e.stats()
    net = e.obs_network(i, j, r, loc, log_cycles=1)
    net.set_values(rng.standard_normal(20))
    e.stats_begin()
    e.assimilate_local(net, inflation=1.05, truth_member=1, record=True)
    seen = e.stats_wait()
    mid = e.download_all()
    assert exact_bits(seen.mean, before.mean) and exact_bits(seen.var, before.var)
    assert not same_bits(mid, S) and exact_bits(mid[1], S[1])
    assert not exact_bits(e.stats().mean, before.mean)
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
