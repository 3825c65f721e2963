"""Linear observations on the GPU (csim_obs_network_create_linear), bit for bit against the numpy restatement of the
header text (tests/obsop_restatement.py, its builders pinned by tests/test_ensemble_obsop_host.py): the analysis on the
whole ensemble, observe, the recorded diagnostics and the log; a one-tap network against the point network; what must
not change; errors; the enqueue-only cycle; and an OSSE with footprint observations."""
import numpy as np
import pytest

import obsnet_restatement as obsnet
import obsop_restatement as ref
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

NX, NY, DX, DY, LOC = 40, 28, 1.0, 0.8, 2.0   # support 4: lx = 3 (3 * 1.0 < 4), ly = 4 (4 * 0.8 < 4)
LX, LY = 3, 4


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
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


def ring_mask():
    ring = np.ones((NY + 2, NX + 2), dtype=bool)
    ring[1:-1, 1:-1] = False
    return ring


def network():
    """40 observations: 1, 4, 25 and 64 taps and boxes clipped at corners and sides; anchors on all four edges and in
    all four corners; a repeated cell, negative weights, taps at |di| = lx and |dj| = ly; r per observation"""
    rng = np.random.default_rng(40)
    full = [(a, b) for b in range(-LY, LY + 1) for a in range(-LX, LX + 1)]          # the 63 cells of a window
    per, i, j = [], [], []

    def add(io, jo, taps):
        i.append(io), j.append(jo), per.append(taps)

    add(1, 1, ref.box(NX, NY, 1, 1, 2, 2))                                             # corner: 9 of 25
    add(NX, NY, ref.box(NX, NY, NX, NY, 2, 2))
    add(1, NY, ([0, 1, 0, 1], [0, 0, -1, -1], [0.4, 0.3, 0.2, 0.1]))
    add(NX, 1, ([0], [0], [1.0]))
    add(1, 14, ref.box(NX, NY, 1, 14, 2, 2))                                           # left side: 15 of 25
    add(NX, 10, ([0, -1, 0, -1], [0, 0, 1, 1], [0.25, 0.25, 0.25, 0.25]))              # right side
    add(20, 1, ([0, 0, 0], [0, 1, 0], [0.5, 0.75, -0.25]))                             # bottom: a repeated cell, w < 0
    add(25, NY, ([-LX, LX, 0, 0], [0, 0, -LY, 0], [0.3, 0.3, 0.3, 0.1]))               # top: |di| = lx, |dj| = ly
    wide = full + [(0, 0)]                                                             # 64 taps, the anchor twice
    add(10, 10, ([a for a, _ in wide], [b for _, b in wide], list(rng.uniform(-1.0, 1.0, 64) / 8.0)))
    add(30, 20, ([a for a, _ in wide], [b for _, b in wide], [1.0 / 64.0] * 64))
    add(4, 5, ([LX, -LX], [LY, -LY], [2.0, -1.0]))                                     # both at the window's corners
    while len(i) < 40:
        kind = len(i) % 4
        if kind == 0:
            io, jo = int(rng.integers(1, NX + 1)), int(rng.integers(1, NY + 1))
            add(io, jo, ([0], [0], [1.0] if len(i) % 8 else [0.5]))
        elif kind == 1:
            io, jo, *t = ref.bilinear(NX, NY, rng.uniform(1, NX), rng.uniform(1, NY))
            add(io, jo, tuple(t))
        elif kind == 2:
            io, jo = int(rng.integers(3, NX - 1)), int(rng.integers(3, NY - 1))
            add(io, jo, ref.box(NX, NY, io, jo, 2, 2))                                 # 25 taps
        else:
            io, jo = int(rng.integers(1, NX + 1)), int(rng.integers(1, NY + 1))
            add(io, jo, ref.box(NX, NY, io, jo, 1, 1))                                 # 3 x 3, clipped where it must be
    i, j = np.array(i, dtype=np.int32), np.array(j, dtype=np.int32)
    taps = ref.concat(per)
    assert ref.check(NX, NY, LX, LY, i, j, taps)
    assert {1, 4, 9, 15, 25, 64} <= set(np.diff(taps[0]).tolist())
    return i, j, taps, rng.uniform(0.05, 1.0, len(i))


@pytest.fixture(scope="module")
def net40(csim):
    i, j, taps, r = network()
    rho = csim.ensemble_gc_table(DX, DY, LOC, NX, NY)
    assert rho.shape == (2 * LY + 1, 2 * LX + 1)
    lev = {o: csim.ensemble_assim_plan(i, j, LX, LY, bool(o)) for o in (0, 1)}
    assert lev[0].max() + 1 >= 3 and lev[1].max() + 1 >= 3
    return dict(i=i, j=j, taps=taps, r=r, rho=rho, lev=lev)


def ensemble(csim, X, bcs="dddd"):
    e = csim.Ensemble(X.shape[0], NX, NY, DX, DY, csim.bc_codes(bcs), 0.5)
    e.upload_all(X)
    return e


# ---- the analysis ---------------------------------------------------------------------------------------------------

# every M (2: the least; 5; 64 and 65: one and two tiles of the linear prior, the register and the re-read form of the
# update; 130: three tiles) with and without a truth member, both orders and both inflations, rotated
CASES = [(2, False, 0, 1.0), (2, True, 1, 1.1), (5, True, 0, 1.1), (5, False, 1, 1.0), (64, True, 1, 1.0),
         (64, False, 0, 1.1), (65, False, 1, 1.1), (65, True, 0, 1.0), (130, True, 1, 1.1), (130, False, 0, 1.0)]


@pytest.mark.parametrize("M,with_truth,ordered,lam", CASES,
                         ids=[f"M{c[0]}_t{int(c[1])}_ord{c[2]}_lam{c[3]}" for c in CASES])
def test_analysis_bits_against_the_restatement(csim, net40, M, with_truth, ordered, lam):
    B = M + 1 if with_truth else M
    t = B // 2 if with_truth else None
    rng = np.random.default_rng(1000 + M)
    X = rng.standard_normal((B, NY + 2, NX + 2))
    y = rng.standard_normal(40)
    i, j, taps, r = net40["i"], net40["j"], net40["taps"], net40["r"]
    e = ensemble(csim, X)
    net = e.obs_network(i, j, r, LOC, ordered=bool(ordered), taps=taps)
    assert net.info == (40, net40["lev"][ordered].max() + 1, LX, LY) and net.ntaps == taps[0][-1]
    net.set_values(y)
    e.assimilate_network(net, inflation=lam, truth_member=t)
    A = e.download_all()
    e.close()
    want = ref.analysis(X, net40["rho"], net40["lev"][ordered], i, j, taps, y, r, lam, t)
    assert same_bits(A, want) and not same_bits(A, X)
    assert exact_bits(A[:, ring_mask()], X[:, ring_mask()])
    if t is not None:
        assert exact_bits(A[t], X[t])


def test_one_tap_network_is_the_point_network(csim):
    """taps (0, 0, 1.0) on a field without zeros: the ensemble after the analysis and every fetched diagnostic equal
    those of a point network on the same cells, bit for bit"""
    B, t = 9, 4
    rng = np.random.default_rng(3)
    X = rng.standard_normal((B, NY + 2, NX + 2))
    assert (X != 0).all()
    i, j = rng.integers(1, NX + 1, 40).astype(np.int32), rng.integers(1, NY + 1, 40).astype(np.int32)
    i[:4], j[:4] = [1, NX, 1, NX], [1, NY, NY, 1]
    r = rng.uniform(0.05, 1.0, 40)
    one = (np.arange(41, dtype=np.int32), np.zeros(40, dtype=np.int32), np.zeros(40, dtype=np.int32), np.ones(40))
    got = []
    for taps in (None, one):
        e = ensemble(csim, X)
        net = e.obs_network(i, j, r, LOC, log_cycles=1, taps=taps)
        net.observe(t, 17, 2)
        e.assimilate_network(net, inflation=1.1, truth_member=t, record=True)
        got.append((e.download_all(), net.fetch(), net.log(), net.ntaps))
        e.close()
    (Ap, fp, lp, np_), (Al, fl, ll, nl) = got
    assert (np_, nl) == (0, 40)
    assert exact_bits(Ap, Al) and not exact_bits(Ap, X)
    for a, b in zip(fp, fl):
        assert exact_bits(a, b)
    assert lp.tobytes() == ll.tobytes()


# ---- observe, the diagnostics and the log ---------------------------------------------------------------------------------

def test_observe_against_the_restatement(csim, net40):
    B, s = 4, 2
    rng = np.random.default_rng(21)
    X = rng.standard_normal((B, NY + 2, NX + 2))
    i, j, taps, r = net40["i"], net40["j"], net40["taps"], net40["r"]
    X[s, 1, NX] = -0.0                          # observation 3, one tap (0, 0, 1.0): +0 + 1.0 * -0 is +0
    e = ensemble(csim, X)
    net = e.obs_network(i, j, r, LOC, taps=taps)
    net.observe(s, 99, 4, noise=False)
    f = net.fetch()
    y, xt = ref.observe(X, s, i, j, taps, r, 99, 4, False)
    assert exact_bits(f.truth, xt) and exact_bits(f.y, xt) and f.y[3] == 0.0 and not np.signbit(f.y[3])
    net.observe(s, 99, 4)
    f = net.fetch()
    y, xt = ref.observe(X, s, i, j, taps, r, 99, 4, True)
    assert exact_bits(f.truth, xt) and exact_bits(f.y, y) and not exact_bits(f.y, f.truth)
    assert exact_bits(f.y, xt + np.sqrt(r) * csim.obs_noise(99, 4, np.arange(40)))      # the noise of the input index
    net.observe(s + 1, 100, 5)
    f = net.fetch()
    y, xt = ref.observe(X, s + 1, i, j, taps, r, 100, 5, True)
    assert exact_bits(f.truth, xt) and exact_bits(f.y, y)
    e.close()


def network_of(rng, nobs):
    """nobs observations of 1, 4, 9 or 25 taps at random anchors"""
    per, i, j = [], [], []
    for o in range(nobs):
        kind = o % 4
        if kind == 1:
            io, jo, *t = ref.bilinear(NX, NY, rng.uniform(1, NX), rng.uniform(1, NY))
            t = tuple(t)
        else:
            io, jo = int(rng.integers(1, NX + 1)), int(rng.integers(1, NY + 1))
            t = ([0], [0], [0.75]) if kind == 0 else ref.box(NX, NY, io, jo, kind - 1, kind - 1)
        i.append(io), j.append(jo), per.append(t)
    return np.array(i, dtype=np.int32), np.array(j, dtype=np.int32), ref.concat(per)


@pytest.mark.parametrize("nobs", [1, 257])
def test_recorded_diagnostics_and_log(csim, nobs):
    """two recorded cycles (values from the host; observed with noise, with inflation): fetch() and log() against the
    restatement; 257 observations are two chunks of the log's sums"""
    B, t = 7, 2
    rng = np.random.default_rng(nobs)
    X = rng.standard_normal((B, NY + 2, NX + 2))
    i, j, taps = network_of(rng, nobs)
    r = rng.uniform(0.05, 1.0, nobs)
    rho = csim.ensemble_gc_table(DX, DY, LOC, NX, NY)
    lev = csim.ensemble_assim_plan(i, j, LX, LY, False)
    e = ensemble(csim, X)
    net = e.obs_network(i, j, r, LOC, log_cycles=2, taps=taps)
    S, want_log = X, []
    for cyc, lam in enumerate((1.0, 1.1)):
        if cyc == 0:
            y, xt = rng.standard_normal(nobs), None
            net.set_values(y)
        else:
            net.observe(t, 7, cyc)
            y, xt = ref.observe(S, t, i, j, taps, r, 7, cyc, True)
        e.assimilate_network(net, inflation=lam, truth_member=t, record=True)
        got = net.fetch()
        hb, vb = ref.mv(S, t, i, j, taps)
        S = ref.analysis(S, rho, lev, i, j, taps, y, r, lam, t)
        ha, va = ref.mv(S, t, i, j, taps)
        assert same_bits(e.download_all(), S)
        assert exact_bits(got.y, y) and (got.truth is None if xt is None else exact_bits(got.truth, xt))
        assert same_bits(got.bg_mean, hb) and same_bits(got.bg_var, vb)
        assert same_bits(got.post_mean, ha) and same_bits(got.post_var, va)
        want_log.append(obsnet.cycle(y, hb, vb, ha, va, r, xt))
    log = net.log()
    assert len(log) == 2 and [row["has_truth"] for row in log] == [0.0, 1.0] and (log["n"] == nobs).all()
    for row, rec in zip(log, want_log):
        assert all(exact_bits(row[f], rec[f]) for f in obsnet.FIELDS), (row, rec)
    e.close()


# ---- what must not change ---------------------------------------------------------------------------------------------

def test_what_must_not_change(csim, net40):
    """the ghost rings, the truth member and every cell outside all windows keep their bits; the buffer that is not
    current cannot be downloaded: what a later run reads of it is its ghost ring, which periodic sides keep for good,
    so a run after the analysis continues every member as a Stepper does from the downloaded state"""
    B, t = 5, 1
    rng = np.random.default_rng(8)
    X = rng.standard_normal((B, NY + 2, NX + 2))
    keep = slice(0, 12)                        # the first 12 observations leave part of the domain outside all windows
    i, j, r = net40["i"][keep], net40["j"][keep], net40["r"][keep]
    start = net40["taps"][0][:13]
    taps = (start, *[a[:start[-1]] for a in net40["taps"][1:]])
    phys = (0.05, 0.1, 0.5, -0.25)
    e = ensemble(csim, X, "pppp")
    e.set_physics(*phys)
    e.run(3)                                   # both buffers have been current
    before = e.download_all()
    net = e.obs_network(i, j, r, LOC, taps=taps)
    net.observe(t, 5, 0)
    e.assimilate_network(net, inflation=1.0, truth_member=t)
    mid = e.download_all()
    inside = ref.windows((NY + 2, NX + 2), net40["rho"], i, j)
    assert inside.any() and not inside[1:-1, 1:-1].all()
    assert not exact_bits(mid, before)
    assert exact_bits(mid[:, ~inside], before[:, ~inside])          # the ghost rings are outside every window
    assert exact_bits(mid[:, ring_mask()], before[:, ring_mask()]) and exact_bits(mid[t], before[t])
    e.run(3)
    got = e.download_all()
    e.close()
    for m in range(B):
        st = csim.Stepper.single(NX, NY, DX, DY, csim.bc_codes("pppp"), 0.5)
        st.upload(mid[m])
        st.run(*phys, 3)
        want = st.download()
        st.close()
        assert same_bits(got[m], want), f"member {m}"


# ---- errors -----------------------------------------------------------------------------------------------------------

def code_of(csim, call):
    with pytest.raises(csim.CsimError) as ei:
        call()
    return ei.value.code


def test_errors_leave_everything_as_it_was(csim):
    """each invalid input of csim_obs_linear_check, through create_linear: CSIM_ERR_ARG, and the ensemble's checksum
    and an existing network's values are as they were"""
    import test_ensemble_obsop_host as host   # the valid set and its violations, on the same 40 x 28 grid

    B = 4
    rng = np.random.default_rng(13)
    X = rng.standard_normal((B, NY + 2, NX + 2))
    e = csim.Ensemble(B, NX, NY, 1.0, 1.0, (0, 0, 0, 0))      # loc 2.0 with dx = dy = 1: lx = ly = 3
    e.upload_all(X)
    i, j, taps = host.valid_set()
    assert host.LY == 3
    ok = [a.copy() for a in taps]
    ok[1] = np.clip(ok[1], -3, 3)               # the valid set's taps at |di| = 5 move to this network's lx = 3
    r = np.array([0.5, 0.25, 1.0, 0.1])
    net = e.obs_network(i, j, r, 2.0, taps=ok)
    assert net.info == (4, 2, 3, 3) and net.ntaps == 78
    net.observe(0, 3, 0)
    y0, sums0 = net.fetch().y, e.checksums()
    for what in host.VIOLATIONS:
        bi, bj, (start, di, dj, w) = host.mutated(what)
        di = np.clip(di, -3, 3)
        if what == "di = lx + 1":
            di[0] = 4
        assert code_of(csim, lambda: e.obs_network(bi, bj, r, 2.0, taps=(start, di, dj, w))) == 1, what
    for kw in (dict(r=[0.0, 1.0, 1.0, 1.0]), dict(loc=-1.0), dict(log_cycles=-1)):
        args = dict(i=i, j=j, r=r, loc=2.0, taps=ok)
        args.update(kw)
        assert code_of(csim, lambda: e.obs_network(**args)) == 1
    assert len(e._nets) == 1 and e.checksums() == sums0
    assert exact_bits(net.fetch().y, y0) and exact_bits(e.download_all(), X)
    e.close()


# ---- the whole cycle, enqueued ------------------------------------------------------------------------------------------

def test_enqueue_only_cycle(csim):
    """run -> observe -> prior_capture -> assimilate_network(record) -> relax -> perturb, two cycles with a box-tap
    network and no host call in between, against the same calls with a sync after each"""
    B = 9
    rng = np.random.default_rng(11)
    X = rng.standard_normal((B, NY + 2, NX + 2))
    I, J = np.meshgrid(np.arange(3, NX, 5), np.arange(3, NY, 5))
    i, j, taps = csim.box_taps(NX, NY, I.ravel(), J.ravel(), 1, 1)
    runs, logs = [], []
    for synced in (False, True):
        e = ensemble(csim, X, "dnpd")
        e.set_physics(0.05, 0.1, 0.5, -0.25)
        net = e.obs_network(i, j, 0.3, LOC, log_cycles=2, taps=taps)
        for cyc in range(2):
            for step in (lambda: e.run(4), lambda: net.observe(0, 31, cyc),
                         lambda: e.prior_capture("spread", truth_member=0),
                         lambda: e.assimilate_network(net, truth_member=0, record=True),
                         lambda: e.relax(0.6, truth_member=0),
                         lambda: e.perturb(0.05, 2.0, 31, cyc, centered=True, truth_member=0)):
                step()
                if synced:
                    e.sync()
        runs.append(e.download_all())
        logs.append(net.log())
        e.close()
    assert same_bits(runs[0], runs[1]) and not same_bits(runs[0][1:], X[1:])
    assert len(logs[0]) == 2 and logs[0].tobytes() == logs[1].tobytes()
    assert (logs[0]["n"] == len(i)).all() and (logs[0]["has_truth"] == 1).all()


# ---- an OSSE with footprints ----------------------------------------------------------------------------------------

def osse_setup():
    """a smooth truth (member 0) and 16 forecast members that are the truth plus smooth errors; 3 x 3 footprints every
    third cell of the left half.  Seed and sizes chosen with the restatement alone (analysis() below on the CPU): there
    the RMSE of the ensemble mean against the truth over the left half falls from 0.2496 to 0.0704."""
    rng = np.random.default_rng(2)
    B = 17
    jj, ii = np.meshgrid(np.arange(NY + 2), np.arange(NX + 2), indexing="ij")
    X = np.empty((B, NY + 2, NX + 2))
    X[0] = np.sin(2 * np.pi * ii / NX) * np.cos(2 * np.pi * jj / NY)
    for k in range(1, B):
        a, b, c = rng.standard_normal(3) * 0.3
        X[k] = X[0] + a + b * np.sin(2 * np.pi * ii / NX + k) + c * np.cos(2 * np.pi * jj / NY - k)
    I, J = np.meshgrid(np.arange(2, NX // 2, 3), np.arange(2, NY, 3))
    return X, I.ravel().astype(np.int32), J.ravel().astype(np.int32)


def left_half_rmse(X):
    mean = np.zeros(X.shape[1:])
    for k in range(1, X.shape[0]):
        mean = mean + X[k]
    mean = mean / (X.shape[0] - 1.0)
    d = (mean - X[0])[1:-1, 1:NX // 2 + 1]
    return float(np.sqrt((d * d).mean()))


def test_osse_footprints_reduce_the_error(csim):
    X, i, j = osse_setup()
    i, j, taps = csim.box_taps(NX, NY, i, j, 1, 1)
    r = 0.01
    e = ensemble(csim, X)
    net = e.obs_network(i, j, r, LOC, log_cycles=1, taps=taps)
    net.observe(0, 77, 0)
    e.assimilate_network(net, truth_member=0, record=True)
    A = e.download_all()
    y = net.fetch().y
    e.close()
    rho = csim.ensemble_gc_table(DX, DY, LOC, NX, NY)
    lev = csim.ensemble_assim_plan(i, j, LX, LY, False)
    y_ref = ref.observe(X, 0, i, j, taps, r, 77, 0, True)[0]
    assert exact_bits(y, y_ref)
    want = ref.analysis(X, rho, lev, i, j, taps, y_ref, np.full(len(i), r), 1.0, 0)
    before, after, after_ref = left_half_rmse(X), left_half_rmse(A), left_half_rmse(want)
    print(f"left-half RMSE of the mean against the truth: {before:.4f} -> {after:.4f} (restatement {after_ref:.4f})")
    assert after_ref < before          # the reference alone shows the decrease
    assert after < before
