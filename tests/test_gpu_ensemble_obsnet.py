"""Observation networks on the GPU (csim_obs_network_*, csim_ensemble_assimilate_network), bit for bit: the analysis
against csim_ensemble_assimilate on a copy of the state; observe, the diagnostics and the log against the numpy
restatement (tests/obsnet_restatement.py, pinned by tests/test_ensemble_obsnet_host.py); the whole cycle enqueued
against the same with a sync after every call and against the host loop; stepping parity; errors and state; an OSSE."""
import numpy as np
import pytest

import obsnet_restatement as ref
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu


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


def make_obs(rng, nx, ny, n):
    """random interior cells, with corners, edges and a duplicated cell when there is room; r per observation"""
    i, j = rng.integers(1, nx + 1, n), rng.integers(1, ny + 1, n)
    if n >= 8:
        i[:6] = [1, nx, 1, nx, 1, (nx + 1) // 2]
        j[:6] = [1, ny, ny, 1, (ny + 1) // 2, 1]
        i[6], j[6] = i[0], j[0]
    return i.astype(np.int32), j.astype(np.int32), rng.uniform(0.05, 2.0, n)


def log_matches(log_row, rec):
    return all(exact_bits(log_row[f], rec[f]) for f in ref.FIELDS)


PHYS = [(0.05, 0.1, 0.5, -0.25), (0.02, 0.1, -0.3, 0.4), (0.08, 0.05, 0.0, 0.0), (0.01, 0.1, 0.2, 0.2),
        (0.03, 0.1, -0.2, -0.1)]


def physics(B):
    return [[PHYS[m % len(PHYS)][k] for m in range(B)] for k in range(4)]


# ---- the same analysis ----------------------------------------------------------------------------------------------

FORECAST = [3, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 130]
GRIDS = [(70, 45), (37, 29), (96, 64), (45, 70)]  # nx, ny
BCS = ["dddd", "pppp", "nnnn", "dnpd"]
# every M (each register step of the update on both sides, and the re-read form) with a truth choice, an order, an
# inflation, sides and a grid, rotated so that each of those meets small and large ensembles
CASES = [(M, n % 2 == 1, n % 4 >= 2, [1.0, 1.05][(n // 2 + n) % 2], BCS[n % 4], GRIDS[(n // 2) % 4])
         for n, M in enumerate(FORECAST)]
CASES += [(64, True, True, 1.05, "pppp", (96, 64)), (65, False, False, 1.0, "nnnn", (37, 29)),
          (4, True, False, 1.05, "dnpd", (45, 70)), (130, True, True, 1.0, "dddd", (37, 29))]


@pytest.mark.parametrize("case", CASES, ids=[f"M{c[0]}_t{int(c[1])}_ord{int(c[2])}_lam{c[3]}_{c[4]}_{c[5][0]}x{c[5][1]}"
                                             for c in CASES])
def test_same_analysis_as_assimilate(csim, case):
    """set_values(y), assimilate_network against csim_ensemble_assimilate on a copy of the same lived-in state: every
    member, ghost ring and truth member included, and again after a run, which reads the ghost rings of the buffer
    that was not current"""
    M, with_truth, ordered, lam, bcs, (nx, ny) = case
    B = M + 1 if with_truth else M
    t = B // 2 if with_truth else None
    rng = np.random.default_rng(M * 10 + nx)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, r = make_obs(rng, nx, ny, 60)
    y = rng.standard_normal(60)
    ens = []
    for _ in range(2):
        e = csim.Ensemble(B, nx, ny, 1.0, 0.8, csim.bc_codes(bcs), 0.5)
        e.upload_all(X)
        e.set_physics(*physics(B))
        e.run(5)
        ens.append(e)
    a, b = ens
    before = a.download_all()
    assert exact_bits(before, b.download_all())
    net = a.obs_network(i, j, r, 3.0, ordered=ordered)
    nl = b.assimilate(i, j, y, r, 3.0, inflation=lam, truth_member=t, ordered=ordered, diagnostics=False)
    tab = csim.ensemble_gc_table(1.0, 0.8, 3.0, nx, ny)   # windows of 11 x 15 cells: many of the 60 overlap
    assert net.info == (60, nl, tab.shape[1] // 2, tab.shape[0] // 2) and nl >= 2
    net.set_values(y)
    a.assimilate_network(net, inflation=lam, truth_member=t)
    A, W = a.download_all(), b.download_all()
    assert same_bits(A, W) and not same_bits(A, before)
    ring = np.ones((ny + 2, nx + 2), dtype=bool)
    ring[1:-1, 1:-1] = False
    assert exact_bits(A[:, ring], before[:, ring])
    if t is not None:
        assert exact_bits(A[t], before[t])
    f = net.fetch()
    assert exact_bits(f.y, y) and f.truth is None and f.bg_mean is None and f.post_var is None
    a.run(6), b.run(6)
    assert same_bits(a.download_all(), b.download_all())
    a.close(), b.close()


# ---- observe ----------------------------------------------------------------------------------------------------------

def test_observe_against_the_restatement(csim):
    B, nx, ny, s = 6, 70, 45, 2
    rng = np.random.default_rng(21)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, r = make_obs(rng, nx, ny, 1000)
    X[s, j[11], i[11]] = -0.0
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    e.upload_all(X)
    net = e.obs_network(i, j, r, 2.0)
    net.observe(s, 99, 4, noise=False)
    f = net.fetch()
    assert exact_bits(f.truth, e.download(s)[j, i]) and exact_bits(f.y, f.truth) and np.signbit(f.y[11])
    net.observe(s, 99, 4)
    f = net.fetch()
    y, xt = ref.observe(X, s, i, j, r, 99, 4, True)
    assert exact_bits(f.truth, xt) and exact_bits(f.y, y) and not exact_bits(f.y, f.truth)
    assert exact_bits(f.y, xt + np.sqrt(r) * csim.obs_noise(99, 4, np.arange(1000)))
    # another draw, another seed, another member: other values
    seen = [f.y]
    for src, seed, draw in ((s, 99, 5), (s, 100, 4), (s + 1, 99, 4)):
        net.observe(src, seed, draw)
        got = net.fetch()
        want = ref.observe(X, src, i, j, r, seed, draw, True)
        assert exact_bits(got.y, want[0]) and exact_bits(got.truth, want[1])
        assert all(not exact_bits(got.y, v) for v in seen)
        seen.append(got.y)
    # the deviate goes with the input index, not with the plan position, the lane or the block: a network of the first
    # 300 observations, and one in the caller's order, have other plans and other launch shapes
    small = e.obs_network(i[:300], j[:300], r[:300], 2.0)
    kept = e.obs_network(i, j, r, 2.0, ordered=True)
    rev = e.obs_network(i[::-1].copy(), j[::-1].copy(), r[::-1].copy(), 2.0)
    for n_ in (small, kept, rev):
        n_.observe(s, 99, 4)
    assert exact_bits(small.fetch().y, f.y[:300]) and exact_bits(kept.fetch().y, f.y)
    # reversed input: the same cells meet the deviates of the other end
    want = ref.observe(X, s, i[::-1], j[::-1], r[::-1], 99, 4, True)
    assert exact_bits(rev.fetch().y, want[0]) and exact_bits(rev.fetch().truth, f.truth[::-1])
    assert net.info.nlevels > 1 and small.info.nlevels <= net.info.nlevels
    e.close()


# ---- diagnostics and the log -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nobs", [1, 255, 256, 257, 5000])
def test_diagnostics_and_log(csim, nobs):
    """three recorded cycles (values from the host, observed with noise, the same values again with inflation): bg_*
    and the log against the restatement, post_* and the members against csim_ensemble_assimilate on a copy"""
    B, t, nx, ny, loc = 10, 3, 128, 96, 1.2
    rng = np.random.default_rng(nobs)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, r = make_obs(rng, nx, ny, nobs)
    a, b = [csim.Ensemble(B, nx, ny, 1.0, 1.0, csim.bc_codes("dnpd")) for _ in range(2)]
    for e in (a, b):
        e.upload_all(X)
        e.set_physics(0.05, 0.1, 0.5, -0.25)
    net = a.obs_network(i, j, r, loc, log_cycles=4)
    want_log = []
    y = rng.standard_normal(nobs)
    for cyc, lam in enumerate((1.0, 1.0, 1.05)):
        a.run(2), b.run(2)
        S = a.download_all()
        xt = None
        if cyc == 0:
            net.set_values(y)
        elif cyc == 1:
            net.observe(t, 7, cyc)
            y, xt = ref.observe(S, t, i, j, r, 7, cyc, True)
        else:
            xt = xt_kept   # the values and their truth are kept
        a.assimilate_network(net, inflation=lam, truth_member=t, record=True)
        got = net.fetch()
        an = b.assimilate(i, j, y, r, loc, inflation=lam, truth_member=t)
        hb, vb = ref.mv(S, t, i, j)
        assert exact_bits(got.y, y)
        assert same_bits(got.bg_mean, hb) and same_bits(got.bg_var, vb)
        assert same_bits(got.post_mean, an.post_mean) and same_bits(got.post_var, an.post_var)
        assert same_bits(a.download_all(), b.download_all())
        if xt is None:
            assert got.truth is None
        else:
            assert exact_bits(got.truth, xt)
            xt_kept = xt
        want_log.append(ref.cycle(y, hb, vb, an.post_mean, an.post_var, r, xt))
    log = net.log()
    assert len(log) == 3
    for row, rec in zip(log, want_log):
        assert log_matches(row, rec), (row, rec)
    assert [row["has_truth"] for row in log] == [0.0, 1.0, 1.0] and (log["n"] == nobs).all()
    assert log["sum_eb2"][0] == 0.0 and log["sum_ea2"][1] > 0.0
    a.close(), b.close()


# ---- the whole cycle, enqueued -----------------------------------------------------------------------------------------

def test_whole_cycle_enqueued(csim):
    """six cycles of run(5) -> observe -> prior_capture -> assimilate_network(record) -> relax -> perturb with no host
    call in between, against (i) the same with a sync after every call and (ii) the host loop of download, obs_noise
    and csim_ensemble_assimilate; a stats_begin before observe and the analysis sees the state before them"""
    B, nx, ny, loc, seed = 12, 96, 64, 4.0, 31
    rng = np.random.default_rng(11)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, r = make_obs(rng, nx, ny, 60)
    runs, logs, caps = [], [], []
    for form in ("enqueued", "synced", "host"):
        e = csim.Ensemble(B, nx, ny, 1.0, 1.0, csim.bc_codes("dnpd"))
        e.upload_all(X)
        e.set_physics(0.05, 0.1, 0.5, -0.25)
        net = e.obs_network(i, j, r, loc, log_cycles=6) if form != "host" else None
        for cyc in range(6):
            if form == "host":
                e.run(5)
                if cyc == 5:
                    caps.append(e.stats())
                truth = e.download(0)
                y = truth[j, i] + np.sqrt(r) * csim.obs_noise(seed, cyc, np.arange(60))
                e.prior_capture("spread", truth_member=0)
                e.assimilate(i, j, y, r, loc, truth_member=0, diagnostics=False)
                e.relax(0.6, truth_member=0)
                e.perturb(0.05, 3.0, seed, cyc, centered=True, truth_member=0)
                continue
            steps = [lambda: e.run(5)]
            if cyc == 5:
                steps.append(lambda: e.stats_begin())
            steps += [lambda: net.observe(0, seed, cyc), lambda: e.prior_capture("spread", truth_member=0),
                      lambda: e.assimilate_network(net, truth_member=0, record=True),
                      lambda: e.relax(0.6, truth_member=0),
                      lambda: e.perturb(0.05, 3.0, seed, cyc, centered=True, truth_member=0)]
            for step in steps:
                step()
                if form == "synced":
                    e.sync()
        runs.append(e.download_all())
        if net is not None:
            caps.append(e.stats_wait())
            logs.append(net.log())
        e.close()
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])
    assert not same_bits(runs[0][1:], X[1:])
    assert len(logs[0]) == 6 and logs[0].tobytes() == logs[1].tobytes()
    assert (logs[0]["n"] == 60).all() and (logs[0]["has_truth"] == 1).all()
    for cap in caps[:2]:
        assert same_bits(cap.mean, caps[2].mean) and same_bits(cap.var, caps[2].var)


# ---- stepping parity ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fuse", [-1, 0])
@pytest.mark.parametrize("bcs", ["dddd", "nnnn", "dnpd"])
def test_analysis_then_run_matches_stepper(csim, bcs, fuse):
    bc = csim.bc_codes(bcs)
    B, nx, ny = 5, 70, 45
    rng = np.random.default_rng(3)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, r = make_obs(rng, nx, ny, 12)
    e = csim.Ensemble(B, nx, ny, 1.0, 0.8, bc, 0.5)
    e.set_option("fuse", fuse)
    e.upload_all(X)
    e.set_physics(*physics(B))
    e.run(4)
    net = e.obs_network(i, j, r, 4.0, log_cycles=1)
    before = e.download_all()
    net.observe(1, 5, 0)
    e.assimilate_network(net, inflation=1.05, truth_member=1, record=True)
    mid = e.download_all()
    assert not same_bits(mid, before) and exact_bits(mid[1], before[1])
    e.run(7)   # from the ensemble's own buffers: nothing is uploaded again
    got = e.download_all()
    e.close()
    for m in range(B):
        st = csim.Stepper.single(nx, ny, 1.0, 0.8, bc, 0.5)
        st.upload(mid[m])
        st.run(*PHYS[m], 7)
        want = st.download()
        st.close()
        assert same_bits(got[m], want), f"member {m}, {bcs}"


# ---- errors and state --------------------------------------------------------------------------------------------------

def code_of(csim, call):
    with pytest.raises(csim.CsimError) as ei:
        call()
    return ei.value.code


def test_create_errors(csim):
    e = csim.Ensemble(4, 8, 6, 1.0, 1.0, (0, 0, 0, 0))
    ok = dict(i=[1, 8], j=[1, 6], r=[1.0, 0.5], loc=2.0)

    def rejected(code=1, **kw):
        args = dict(ok)
        args.update(kw)
        assert code_of(csim, lambda: e.obs_network(**args)) == code, kw

    for kw in (dict(i=[0, 8]), dict(i=[1, 9]), dict(j=[1, 7]), dict(j=[0, 6]), dict(r=[0.0, 1.0]), dict(r=[-1.0, 1.0]),
               dict(r=[np.inf, 1.0]), dict(r=[np.nan, 1.0]), dict(loc=0.0), dict(loc=-1.0), dict(loc=np.inf),
               dict(loc=np.nan), dict(log_cycles=-1), dict(log_cycles=65537), dict(i=[], j=[], r=[])):
        rejected(**kw)
    L, C = csim.lib(), csim.C
    out = C.c_void_p()
    ii, rr = (C.c_int * 1)(1), (C.c_double * 1)(1.0)
    raw = lambda n, i_, j_, r_, ordered=0, o=C.byref(out): L.csim_obs_network_create(e._h, n, i_, j_, r_, 2.0, ordered, 0, o)
    assert raw(1, ii, ii, rr, 2) == 1 and raw(1, None, ii, rr) == 1 and raw(1, ii, ii, None) == 1
    assert raw(0, ii, ii, rr) == 1 and raw(-1, ii, ii, rr) == 1 and raw(1, ii, ii, rr, 0, None) == 1
    assert raw(2 ** 20 + 1, ii, ii, rr) == 5 and not out.value
    assert len(e._nets) == 0
    net = e.obs_network(log_cycles=65536, **ok)
    assert net.info == (2, 1, 3, 3)
    e.close()


def test_errors_leave_everything_as_it_was(csim):
    B, nx, ny = 5, 24, 16
    rng = np.random.default_rng(8)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, r = make_obs(rng, nx, ny, 20)
    y = rng.standard_normal(20)
    e, other = [csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0)) for _ in range(2)]
    e.upload_all(X), other.upload_all(X)
    net = e.obs_network(i, j, r, 2.0, log_cycles=2)
    nolog = e.obs_network(i, j, r, 2.0)
    foreign = other.obs_network(i, j, r, 2.0)
    L = csim.lib()
    unchanged = lambda: exact_bits(e.download_all(), X)
    # no values yet
    assert code_of(csim, lambda: e.assimilate_network(net)) == 4
    assert L.csim_obs_network_fetch(net._h, csim._dp(np.empty(20)), None, None, None, None, None) == 4
    assert net.fetch() == (None,) * 6 and unchanged()
    bad = y.copy()
    bad[7] = np.nan
    assert code_of(csim, lambda: net.set_values(bad)) == 1
    bad[7] = np.inf
    assert code_of(csim, lambda: net.set_values(bad)) == 1
    assert code_of(csim, lambda: e.assimilate_network(net)) == 4   # still none
    with pytest.raises(ValueError):
        net.set_values(y[:5])
    net.set_values(y)
    foreign.set_values(y), nolog.set_values(y)
    for call in (lambda: net.observe(-1, 1), lambda: net.observe(B, 1), lambda: net.observe(0, 1, noise=2),
                 lambda: net.observe(0, 1, noise=-1)):
        assert code_of(csim, call) == 1
    f = net.fetch()
    assert exact_bits(f.y, y) and f.truth is None   # a refused observe kept the values and has_truth
    assert L.csim_obs_network_fetch(net._h, None, csim._dp(np.empty(20)), None, None, None, None) == 4
    assert L.csim_obs_network_fetch(net._h, None, None, None, None, csim._dp(np.empty(20)), None) == 4
    calls = [(lambda: e.assimilate_network(net, inflation=0.99), 1), (lambda: e.assimilate_network(net, inflation=np.nan), 1),
             (lambda: e.assimilate_network(net, inflation=np.inf), 1), (lambda: e.assimilate_network(net, truth_member=B), 1),
             (lambda: e.assimilate_network(net, truth_member=-2), 1), (lambda: e.assimilate_network(net, record=2), 1),
             (lambda: e.assimilate_network(net, record=-1), 1), (lambda: e.assimilate_network(foreign), 1),
             (lambda: other.assimilate_network(net), 1), (lambda: e.assimilate_network(nolog, record=True), 4)]
    for call, code in calls:
        assert code_of(csim, call) == code
    assert unchanged() and exact_bits(other.download_all(), X) and len(net.log()) == 0
    assert exact_bits(net.fetch().y, y)
    # the values serve several analyses; the log fills up and is reset
    ref_e = csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    ref_e.upload_all(X)
    for _ in range(2):
        e.assimilate_network(net, record=True)
        ref_e.assimilate(i, j, y, r, 2.0, diagnostics=False)
        assert same_bits(e.download_all(), ref_e.download_all())
    S = e.download_all()
    assert not exact_bits(S, X)
    assert code_of(csim, lambda: e.assimilate_network(net, record=True)) == 4   # the log is full
    assert exact_bits(e.download_all(), S) and len(net.log()) == 2
    first = net.log()
    e.assimilate_network(net)                                                   # without a record it still runs
    ref_e.assimilate(i, j, y, r, 2.0, diagnostics=False)
    assert same_bits(e.download_all(), ref_e.download_all()) and net.log().tobytes() == first.tobytes()
    net.log_reset()
    assert len(net.log()) == 0
    S = e.download_all()
    hb, vb = ref.mv(S, None, i, j)
    e.assimilate_network(net, record=True)
    an = ref_e.assimilate(i, j, y, r, 2.0)
    log = net.log()
    assert len(log) == 1 and log_matches(log[0], ref.cycle(y, hb, vb, an.post_mean, an.post_var, r))
    assert first["sum_vb"][0] != log["sum_vb"][0]
    ref_e.close()
    # M < 2 and M > CSIM_ASSIM_MAX_MEMBERS
    two = csim.Ensemble(2, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    n2 = two.obs_network(i, j, r, 2.0)
    n2.set_values(y)
    assert code_of(csim, lambda: two.assimilate_network(n2, truth_member=0)) == 1
    two.assimilate_network(n2)
    two.close()
    big = csim.Ensemble(1026, 4, 4, 1.0, 1.0, (0, 0, 0, 0))
    nb = big.obs_network([1, 4], [2, 3], 1.0, 2.0)
    nb.set_values([0.5, -0.5])
    assert code_of(csim, lambda: big.assimilate_network(nb)) == 5
    assert code_of(csim, lambda: big.assimilate_network(nb, truth_member=3)) == 5
    big.close()
    # destroying the ensemble takes its networks along; a closed network is refused, closing it again is harmless
    e.close()
    assert net._h is None and nolog._h is None and len(e._nets) == 0
    net.close()
    assert code_of(csim, lambda: other.assimilate_network(net)) == 1
    foreign.close()
    assert len(other._nets) == 0
    other.close()


def test_network_collected_together_with_its_ensemble(csim):
    """An ensemble and its network, neither closed, freed by the cyclic collector in one go, as after a failed test
    whose traceback keeps both.  The collector clears the ensemble's weak references to its networks before it runs
    either __del__, so the ensemble cannot clear the network's handle: the network itself must see that its ensemble
    is closed, and not hand the library a network that went with the ensemble"""
    import gc
    import weakref

    e = csim.Ensemble(3, 8, 6, 1.0, 1.0, (0, 0, 0, 0))
    net = e.obs_network([1, 8], [1, 6], 1.0, 2.0)
    e.keeps = net                       # the ensemble reaches its network: one cycle, unreachable after the del
    gone = weakref.ref(e)
    del e, net
    gc.collect()
    assert gone() is None
    # the other order, by hand: the ensemble first, then a network whose handle it could not clear
    e = csim.Ensemble(3, 8, 6, 1.0, 1.0, (0, 0, 0, 0))
    net = e.obs_network([1, 8], [1, 6], 1.0, 2.0)
    e._nets.clear()
    e.close()
    assert net._h is not None
    net.close()
    assert net._h is None
    # the library goes on working
    e = csim.Ensemble(3, 8, 6, 1.0, 1.0, (0, 0, 0, 0))
    e.upload_all(np.random.default_rng(0).standard_normal((3, 8, 10)))
    net = e.obs_network([1, 8], [1, 6], 1.0, 2.0)
    net.set_values([0.5, -0.5])
    e.assimilate_network(net)
    assert np.isfinite(e.download_all()).all()
    e.close()


# ---- an OSSE with observations on the left half of the domain --------------------------------------------------------

def test_osse_with_half_the_domain_observed_by_a_network(csim):
    """The set-up of test_osse_with_half_the_domain_observed (tests/test_gpu_ensemble_relax.py), driven by a network:
    six cycles of run -> observe -> capture -> analysis -> relax, one log at the end.  Asserted per cycle is
    only what the definitions give: the truth member keeps its bits, without inflation sum_va <= sum_vb (every rank-1
    update of the filter takes variance away from every cell it touches), and n.  RMSE, spread and the Desroziers
    ratio sum_oa_ob / sum_r are printed."""
    B, nx, ny, sigma0, corr, alpha = 33, 96, 96, 0.05, 5.0, 0.7
    e, free = [csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0)) for _ in range(2)]
    for x in (e, free):
        for m in range(B):
            x.init_gaussian(m, 1.0, 0.08, 0.5, 0.5)
        x.set_physics(0.05, 0.1, 0.3, 0.1)
        x.perturb(sigma0, corr, 2025, 0)
    I, J = np.meshgrid(np.arange(2, nx // 2, 4), np.arange(2, ny + 1, 4))
    i, j = I.ravel(), J.ravel()
    r_obs = 0.005
    net = e.obs_network(i, j, r_obs * r_obs, corr, log_cycles=6)
    for cyc in range(1, 7):
        e.run(5), free.run(5)
        truth = e.download(0)
        net.observe(0, 4, cyc)
        e.prior_capture("spread", truth_member=0)
        e.assimilate_network(net, truth_member=0, record=True)
        e.relax(alpha, truth_member=0)
        assert exact_bits(e.download(0), truth)
        assert exact_bits(net.fetch().truth, truth[j, i])
    log = net.log()
    assert len(log) == 6 and (log["n"] == len(i)).all() and (log["has_truth"] == 1).all()
    assert exact_bits(e.download(0), free.download(0))   # the truth member: the same bits as without any analysis
    for cyc, row in enumerate(log, 1):
        n = row["n"]
        print(f"cycle {cyc}: at the observations rmse {np.sqrt(row['sum_eb2'] / n):.6f} -> {np.sqrt(row['sum_ea2'] / n):.6f}, "
              f"spread {np.sqrt(row['sum_vb'] / n):.6f} -> {np.sqrt(row['sum_va'] / n):.6f}, "
              f"Desroziers sum_oa_ob / sum_r {row['sum_oa_ob'] / row['sum_r']:.4f}")
        assert row["sum_va"] <= row["sum_vb"]
    v, vf = e.verify(truth_member=0).scores, free.verify(truth_member=0).scores
    print(f"after six cycles: rmse {v.rmse:.5f} spread {v.spread:.5f}; without analyses rmse {vf.rmse:.5f} "
          f"spread {vf.spread:.5f}")
    e.close(), free.close()
