"""Relaxation inflation (csim_ensemble_prior_capture / csim_ensemble_relax) on the GPU against the numpy restatement of
the block in include/csim.h (tests/relax_restatement.py, pinned to closed forms by tests/test_ensemble_relax_host.py),
bit for bit; the identity outside the observation windows; what the relaxation is for; pipelining and stepping parity;
the validity rules and the errors; and an OSSE with observations on half of the domain."""
import numpy as np
import pytest

import relax_restatement as ref
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
    """the same 64-bit patterns; a NaN must meet a NaN, but matches any NaN, as in tests/test_gpu_ensemble_assim.py: the
    sign of a NaN that an operation makes (inf - inf, inf / inf) is the hardware's choice and differs between the host
    and the GPU"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.int64), want[ok].view(np.int64))


def ring_mask(ny, nx):
    ring = np.ones((ny + 2, nx + 2), dtype=bool)
    ring[1:-1, 1:-1] = False
    return ring


MODES = {"spread": ref.SPREAD, "pert": ref.PERT}


# ---- the restatement ---------------------------------------------------------------------------------------------

def prior_and_analysis(rng, B, t, ny, nx):
    """a random prior, and an analysis that shrinks, grows and shifts the forecast members on a sub-rectangle of the
    interior and leaves every other bit alone; on grids of at least 16 cells, special cells (see SPECIAL)"""
    X = rng.standard_normal((B, ny + 2, nx + 2))
    A = X.copy()
    ks = ref.forecast(B, t)
    j0, j1 = 1 + ny // 4, 1 + max(ny // 4 + 1, (3 * ny) // 4)
    i0, i1 = 1 + nx // 4, 1 + max(nx // 4 + 1, (3 * nx) // 4)
    c = rng.uniform(0.3, 1.6, (j1 - j0, i1 - i0))  # below 1: shrinks, above: grows
    m = X[ks][:, j0:j1, i0:i1].mean(axis=0)
    for k in ks:
        A[k, j0:j1, i0:i1] = m + c * (X[k, j0:j1, i0:i1] - m) + 0.3
    if nx * ny >= 16:
        cells = [(1 + e // nx, 1 + e % nx) for e in range(1, 2 * len(SPECIAL), 2)]
        for (j, i), special in zip(cells, SPECIAL):
            special(X, A, ks, j, i)
    return X, A


def _agree_after(X, A, ks, j, i):      # sa == 0, sb > 0
    A[ks, j, i] = 0.75


def _agree_before(X, A, ks, j, i):     # sb == 0 with sa > 0: f = -alpha
    X[ks, j, i] = -1.25
    A[ks, j, i] = np.arange(len(ks)) * 0.5


def _zeros(X, A, ks, j, i):            # +-0 in prior and analysis
    X[ks, j, i] = np.where(np.arange(len(ks)) % 2, 0.0, -0.0)
    A[ks, j, i] = np.where(np.arange(len(ks)) % 2, -0.0, 0.0)


def _minus_zero_kept(X, A, ks, j, i):  # untouched -0: must stay -0
    X[ks, j, i] = -0.0
    A[ks, j, i] = -0.0


def _subnormal(X, A, ks, j, i):
    X[ks, j, i] = np.arange(len(ks)) * 3 * 5e-324
    A[ks, j, i] = np.arange(len(ks)) * 5e-324


def _huge(X, A, ks, j, i):             # (x - m)^2 overflows
    X[ks, j, i] = np.where(np.arange(len(ks)) % 2, 1e300, -1e300)
    A[ks, j, i] = np.where(np.arange(len(ks)) % 2, 0.5e300, -1e300)


def _inf(X, A, ks, j, i):
    A[ks[-1], j, i] = np.inf


def _nan(X, A, ks, j, i):
    A[ks[0], j, i] = np.nan


def _nan_before(X, A, ks, j, i):       # NaN sb, sa > 0
    X[ks[len(ks) // 2], j, i] = np.nan
    A[ks, j, i] = np.arange(len(ks)) * 0.25


SPECIAL = [_agree_after, _agree_before, _zeros, _minus_zero_kept, _subnormal, _huge, _inf, _nan, _nan_before]

FORECAST = [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 130, 300]
GRIDS = [(1, 1), (5, 1), (1, 7), (130, 3), (96, 64), (67, 45)]  # nx, ny
ALPHAS = [1.0, 0.5, 0.3]
# each M with one grid, truth choice (none, first, middle, last) and alpha per mode, rotated so that every grid meets
# the register form, the re-read form and every truth choice
CASES = []
for n, M in enumerate(FORECAST):
    for mode, shift in (("spread", 0), ("pert", 1)):
        which = (n + shift) % 4
        t = [None, 0, M // 2, M][which]
        CASES.append((mode, M, t, GRIDS[(n + 2 * shift) % 6], ALPHAS[(n + shift) % 3]))
CASES += [("spread", 64, 64, (96, 64), 0.3), ("pert", 64, None, (96, 64), 0.5), ("spread", 300, 7, (67, 45), 1.0),
          ("pert", 300, 299, (130, 3), 1.0), ("spread", 5, 2, (1, 1), 0.5), ("spread", 1024, None, (5, 1), 0.5)]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}_M{c[1]}_t{c[2]}_{c[3][0]}x{c[3][1]}_a{c[4]}" for c in CASES])
def test_restatement_bit_for_bit(csim, case):
    mode, M, t, (nx, ny), alpha = case
    B = M if t is None else M + 1
    rng = np.random.default_rng(M * 100 + nx)
    X, A = prior_and_analysis(rng, B, t, ny, nx)
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    e.upload_all(X)
    e.prior_capture(mode, truth_member=t)
    e.upload_all(A)                                  # uploads keep the capture valid
    f = e.relax(alpha, mode, truth_member=t, factor=(mode == "spread"))
    got = e.download_all()
    e.close()
    cap = ref.capture(X, MODES[mode], t)
    want, wf = ref.relax(A, cap, MODES[mode], alpha, t)
    assert same_bits(got, want), f"{np.abs(got - want).max()}"
    ring = ring_mask(ny, nx)
    assert np.array_equal(got[:, ring].view(np.int64), A[:, ring].view(np.int64))
    if t is not None:
        assert np.array_equal(got[t].view(np.int64), A[t].view(np.int64))
    assert not np.array_equal(got.view(np.int64), A.view(np.int64))
    if mode == "spread":
        assert same_bits(f, wf)
        assert np.array_equal(f[ring].view(np.int64), np.zeros(ring.sum(), dtype=np.int64))
        # cells the analysis left alone: f is +0 and the bits are the uploaded ones
        ks = ref.forecast(B, t)
        alone = (X[ks].view(np.int64) == A[ks].view(np.int64)).all(axis=0) & ~ring
        assert alone.any() or nx * ny < 4
        assert np.array_equal(f[alone].view(np.int64), np.zeros(alone.sum(), dtype=np.int64))
        assert np.array_equal(got[:, alone].view(np.int64), A[:, alone].view(np.int64))


# ---- identity outside the observation windows ---------------------------------------------------------------------

def outside_windows(csim, nx, ny, i, j, loc, dx=1.0, dy=1.0):
    """interior cells with |di| > lx or |dj| > ly from every observation, as a (ny+2, nx+2) mask"""
    tab = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    ly, lx = tab.shape[0] // 2, tab.shape[1] // 2
    J, I = np.meshgrid(np.arange(ny + 2), np.arange(nx + 2), indexing="ij")
    out = ~ring_mask(ny, nx)
    for io, jo in zip(i, j):
        out &= (np.abs(I - io) > lx) | (np.abs(J - jo) > ly)
    return out


def test_identity_outside_the_windows(csim):
    B, t, nx, ny = 34, 5, 96, 96
    rng = np.random.default_rng(2)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    X[:, 90, 90] = -0.0
    i, j = np.array([10, 40, 41, 80]), np.array([12, 60, 58, 20])
    y = rng.standard_normal(4)
    out = outside_windows(csim, nx, ny, i, j, 3.0)
    assert out.sum() > 0.8 * nx * ny and out[90, 90]
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, csim.bc_codes("dnpd"))
    e.upload_all(X)
    e.prior_capture("spread", truth_member=t)
    e.assimilate(i, j, y, 0.1, 3.0, truth_member=t, diagnostics=False)
    before = e.download_all()
    f = e.relax(1.0, truth_member=t, factor=True)
    after = e.download_all()
    e.close()
    bits = lambda a: a.view(np.int64)
    assert np.array_equal(bits(after[:, out]), bits(before[:, out])) and np.signbit(after[:, 90, 90]).all()
    ring = ring_mask(ny, nx)
    assert np.array_equal(bits(after[:, ring]), bits(before[:, ring]))
    assert np.array_equal(bits(after[t]), bits(before[t]))
    assert np.array_equal(bits(f[out | ring]), np.zeros((out | ring).sum(), dtype=np.int64))
    changed = (bits(after) != bits(before)).any(axis=0)
    assert changed.any() and not changed[out].any() and (f[changed] != 0).all()
    cap = ref.capture(X, ref.SPREAD, t)
    want, wf = ref.relax(before, cap, ref.SPREAD, 1.0, t)
    assert same_bits(after, want) and same_bits(f, wf)


# ---- what it is for ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [5, 33, 64, 200])
@pytest.mark.parametrize("alpha", [1.0, 0.6])
def test_spread_and_perturbations_come_back(csim, M, alpha):
    """RTPS: the spread becomes alpha sb + (1 - alpha) sa and the mean stays; RTPP with alpha = 1: the perturbations
    are the captured ones.  The bounds are rounding bounds: the restatement alone stays below 4e-14 on such data."""
    nx, ny = 40, 24
    rng = np.random.default_rng(M)
    inner = (slice(None), slice(1, -1), slice(1, -1))
    X = rng.standard_normal((M, ny + 2, nx + 2)) + rng.uniform(-3, 3, (ny + 2, nx + 2))
    c = rng.uniform(0.2, 1.0, (ny + 2, nx + 2))
    mb = X.mean(axis=0)
    A = mb + c * (X - mb) + 0.3
    sb, sa = X.std(axis=0, ddof=1), A.std(axis=0, ddof=1)
    e = csim.Ensemble(M, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    e.upload_all(X)
    e.prior_capture("spread")
    e.upload_all(A)
    e.relax(alpha)
    R = e.download_all()
    want_s = alpha * sb + (1 - alpha) * sa
    err_s = np.abs(R.std(axis=0, ddof=1) - want_s)[inner[1:]] / want_s[inner[1:]]
    err_m = (np.abs(R.mean(axis=0) - A.mean(axis=0)) / sb)[inner[1:]]
    print(f"M {M} alpha {alpha}: spread error {err_s.max():.3e} relative, mean moved {err_m.max():.3e} sb")
    assert err_s.max() <= 1e-12 and err_m.max() <= 1e-12
    e.upload_all(X)
    e.prior_capture("pert")
    e.upload_all(A)
    e.relax(1.0, "pert")
    R = e.download_all()
    e.close()
    err_p = (np.abs((R - R.mean(axis=0)) - (X - mb)) / sb)[inner]
    err_m = (np.abs(R.mean(axis=0) - A.mean(axis=0)) / sb)[inner[1:]]
    print(f"M {M}: RTPP perturbation error {err_p.max():.3e} sb, mean moved {err_m.max():.3e} sb")
    assert err_p.max() <= 1e-12 and err_m.max() <= 1e-12


# ---- pipelining and stepping parity ---------------------------------------------------------------------------------

def test_cycle_pipelines_and_captures_see_the_state_before(csim):
    B, nx, ny = 12, 96, 64
    rng = np.random.default_rng(11)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j = rng.integers(1, nx + 1, 60), rng.integers(1, ny + 1, 60)
    y = rng.standard_normal(60)
    for mode in ("spread", "pert"):
        runs = []
        for sync in (False, True):
            e = csim.Ensemble(B, nx, ny, 1.0, 1.0, csim.bc_codes("dnpd"))
            e.upload_all(X)
            e.set_physics(0.05, 0.1, 0.5, -0.25)
            steps = [lambda: e.run(4), lambda: e.prior_capture(mode, truth_member=0),
                     lambda: e.assimilate(i, j, y, 0.5, 4.0, truth_member=0, diagnostics=False)]
            for step in steps:
                step()
                if sync:
                    e.sync()
            s1 = e.stats() if sync else None
            e.stats_begin()
            for step in (lambda: e.relax(0.8, mode, truth_member=0),
                         lambda: e.perturb(0.2, 3.0, 8, 1, centered=True, truth_member=0)):
                if sync:
                    e.sync()
                step()
            if sync:
                e.sync()
            e.run(7)
            runs.append(e.download_all())
            cap = e.stats_wait()
            if sync:
                assert same_bits(cap.mean, s1.mean) and same_bits(cap.var, s1.var)
            else:
                first = cap
            e.close()
        assert same_bits(runs[0], runs[1]), mode
        assert same_bits(first.var, cap.var) and same_bits(first.mean, cap.mean)


PHYS = [(0.05, 0.1, 0.5, -0.25), (0.02, 0.1, -0.3, 0.4), (0.08, 0.05, 0.0, 0.0), (0.01, 0.1, 0.2, 0.2),
        (0.03, 0.1, -0.2, -0.1)]


@pytest.mark.parametrize("fuse", [-1, 0])
@pytest.mark.parametrize("mode", ["spread", "pert"])
@pytest.mark.parametrize("bcs", ["dddd", "nnnn", "pppp", "dnpd"])
def test_relax_then_run_matches_stepper(csim, bcs, mode, fuse):
    bc = csim.bc_codes(bcs)
    B, nx, ny = 5, 70, 45
    rng = np.random.default_rng(3)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j, y = rng.integers(1, nx + 1, 12), rng.integers(1, ny + 1, 12), rng.standard_normal(12)
    e = csim.Ensemble(B, nx, ny, 1.0, 0.8, bc, 0.5)
    e.set_option("fuse", fuse)
    e.upload_all(X)
    e.set_physics(*[[p[k] for p in PHYS] for k in range(4)])
    e.run(4)
    e.prior_capture(mode, truth_member=1)
    e.assimilate(i, j, y, 0.5, 4.0, truth_member=1, diagnostics=False)
    before = e.download_all()
    e.relax(0.7, mode, truth_member=1)
    mid = e.download_all()
    assert not same_bits(mid, before) and same_bits(mid[1], before[1])
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
    # As in test_run_perturb_run_matches_stepper: what a later run reads of the buffer that is not current is its ghost
    # ring, which periodic sides keep for good, so a write there, or into a ghost ring, fails this comparison.


# ---- validity and errors ------------------------------------------------------------------------------------------

def state_error(csim, call):
    with pytest.raises(csim.CsimError) as ei:
        call()
    return ei.value.code


def test_validity(csim):
    B, t, nx, ny = 7, 3, 37, 21
    rng = np.random.default_rng(5)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    A = X.copy()
    A[:, 3:15, 4:30] = 0.5 * A[:, 3:15, 4:30] + 0.1
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    e.set_physics(0.05, 0.1, 0.5, -0.25)
    e.upload_all(A)
    unchanged = lambda: np.array_equal(e.download_all().view(np.int64), A.view(np.int64))
    for mode in ("spread", "pert"):
        assert state_error(csim, lambda: e.relax(0.5, mode, truth_member=t)) == 4      # before any capture
    assert unchanged()
    for mode, other in (("spread", "pert"), ("pert", "spread")):
        e.upload_all(X)
        e.prior_capture(mode, truth_member=t)
        e.upload_all(A)
        assert state_error(csim, lambda: e.relax(0.5, other, truth_member=t)) == 4     # the other mode
        assert state_error(csim, lambda: e.relax(0.5, mode, truth_member=t + 1)) == 4  # another truth member
        assert state_error(csim, lambda: e.relax(0.5, mode)) == 4
        assert unchanged()
        e.relax(0.0, mode, truth_member=t)                                             # alpha = 0: nothing
        assert unchanged()
        cap = ref.capture(X, MODES[mode], t)
        # calls that keep the capture valid; the state is followed on the host through downloads
        e.run(0)
        e.upload(0, A[0])
        e.init_gaussian(t, 1.0, 0.1, 0.5, 0.5)
        e.assimilate([5, 20], [6, 10], [0.3, -0.2], 0.5, 3.0, truth_member=t, diagnostics=False)
        e.perturb(0.05, 2.0, 9, 0, truth_member=t)
        e.stats()
        e.quantiles([0.5])
        e.verify(truth_member=t)
        S = e.download_all()
        e.relax(0.5, mode, truth_member=t)
        one, _ = ref.relax(S, cap, MODES[mode], 0.5, t)
        assert same_bits(e.download_all(), one) and not same_bits(one, S)
        e.relax(0.5, mode, truth_member=t)                                             # relax consumes nothing
        two, _ = ref.relax(one, cap, MODES[mode], 0.5, t)
        assert same_bits(e.download_all(), two) and not same_bits(two, one)
        e.run(1)                                                                       # the forecast is gone
        S = e.download_all()
        assert state_error(csim, lambda: e.relax(0.5, mode, truth_member=t)) == 4
        assert np.array_equal(e.download_all().view(np.int64), S.view(np.int64))
    # a capture of either mode replaces the last one
    e.prior_capture("pert", truth_member=t)
    e.prior_capture("spread", truth_member=t)
    assert state_error(csim, lambda: e.relax(0.5, "pert", truth_member=t)) == 4
    e.relax(0.5, "spread", truth_member=t)
    e.close()


def test_argument_errors(csim):
    nx, ny = 8, 8
    X = np.random.default_rng(6).standard_normal((3, ny + 2, nx + 2))
    e = csim.Ensemble(3, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    e.upload_all(X)
    e.prior_capture("spread", truth_member=0)
    A = X.copy()
    A[1:, 2:6, 2:6] *= 0.5
    e.upload_all(A)
    buf = np.zeros((ny + 2, nx + 2))
    L = csim.lib()
    raw = lambda mode, alpha, t, out=None: L.csim_ensemble_relax(e._h, mode, alpha, t, out)
    bad = [(0, 0.5, 0), (3, 0.5, 0), (-1, 0.5, 0), (1, 0.5, 3), (1, 0.5, -2), (1, np.nan, 0), (1, np.inf, 0),
           (1, -0.1, 0), (1, 1.0000001, 0), (2, 0.5, 0, csim._dp(buf))]
    for args in bad:
        assert raw(*args) == 1, args
    for mode, t in [(0, 0), (3, 0), (1, 3), (1, -2)]:
        assert L.csim_ensemble_prior_capture(e._h, mode, t) == 1, (mode, t)
    assert np.array_equal(e.download_all().view(np.int64), A.view(np.int64))
    # the capture survived the refused calls
    e.relax(1.0, "spread", truth_member=0)
    want, _ = ref.relax(A, ref.capture(X, ref.SPREAD, 0), ref.SPREAD, 1.0, 0)
    assert same_bits(e.download_all(), want) and not same_bits(want, A)
    e.close()
    # M < 2
    two = csim.Ensemble(2, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    one = csim.Ensemble(1, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    for ens, t in ((two, 0), (two, 1), (one, None)):
        for mode in ("spread", "pert"):
            assert state_error(csim, lambda: ens.prior_capture(mode, truth_member=t)) == 1
            assert state_error(csim, lambda: ens.relax(0.5, mode, truth_member=t)) == 1
    two.prior_capture("pert")
    two.relax(1.0, "pert")
    two.close(), one.close()
    # M > CSIM_ASSIM_MAX_MEMBERS
    big = csim.Ensemble(1026, 4, 4, 1.0, 1.0, (0, 0, 0, 0))
    Z = np.random.default_rng(7).standard_normal((1026, 6, 6))
    big.upload_all(Z)
    for t in (None, 3):
        for mode in ("spread", "pert"):
            assert state_error(csim, lambda: big.prior_capture(mode, truth_member=t)) == 5
            assert state_error(csim, lambda: big.relax(0.5, mode, truth_member=t)) == 5
    assert np.array_equal(big.download_all().view(np.int64), Z.view(np.int64))
    big.close()


# ---- an OSSE with observations on the left half of the domain ------------------------------------------------------

def test_osse_with_half_the_domain_observed(csim):
    """The set-up of test_osse_cycles_without_an_upload with observations on the left half only, six cycles of
    run -> analysis for (a) multiplicative inflation, (b) capture -> assimilate -> relax, (c) no inflation, from the same
    bits.  Asserted per cycle is only what the definitions give; RMSE and spread of the three are printed."""
    B, nx, ny, sigma0, corr, lam, alpha = 33, 96, 96, 0.05, 5.0, 1.05, 0.7
    ens = []
    for _ in range(3):
        e = csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
        for m in range(B):
            e.init_gaussian(m, 1.0, 0.08, 0.5, 0.5)
        e.set_physics(0.05, 0.1, 0.3, 0.1)
        e.perturb(sigma0, corr, 2025, 0)
        ens.append(e)
    a, b, c = ens
    assert same_bits(a.download_all(), b.download_all()) and same_bits(a.download_all(), c.download_all())
    I, J = np.meshgrid(np.arange(2, nx // 2, 4), np.arange(2, ny + 1, 4))
    i, j = I.ravel(), J.ravel()
    out = outside_windows(csim, nx, ny, i, j, corr)
    assert out.sum() > 0.3 * nx * ny
    inner = ~ring_mask(ny, nx)
    rng = np.random.default_rng(4)
    r_obs = 0.005
    spread = lambda S: S[1:].std(axis=0, ddof=1)
    bits = lambda S: S.view(np.int64)
    for cyc in range(1, 7):
        for e in ens:
            e.run(5)
        truth = a.download(0)
        assert same_bits(truth, b.download(0)) and same_bits(truth, c.download(0))
        y = truth[j, i] + r_obs * rng.standard_normal(len(i))
        # (a)
        Sa = a.download_all()
        a.assimilate(i, j, y, r_obs * r_obs, corr, inflation=lam, truth_member=0, diagnostics=False)
        Ta = a.download_all()
        ratio = spread(Ta)[out] / spread(Sa)[out]
        print(f"cycle {cyc}: (a) spread ratio outside the windows {ratio.min():.15f} .. {ratio.max():.15f}")
        assert np.abs(ratio / lam - 1.0).max() <= 1e-12
        # (b)
        Sb = b.download_all()
        b.prior_capture("spread", truth_member=0)
        b.assimilate(i, j, y, r_obs * r_obs, corr, truth_member=0, diagnostics=False)
        Tb = b.download_all()
        b.relax(alpha, truth_member=0)
        Rb = b.download_all()
        assert np.array_equal(bits(Rb[:, out]), bits(Sb[:, out]))
        lo, hi = np.minimum(spread(Tb), spread(Sb))[inner], np.maximum(spread(Tb), spread(Sb))[inner]
        got = spread(Rb)[inner]
        assert (got >= lo * (1 - 1e-12)).all() and (got <= hi * (1 + 1e-12)).all()
        assert not np.array_equal(bits(Rb), bits(Tb))
        # (c)
        c.assimilate(i, j, y, r_obs * r_obs, corr, truth_member=0, diagnostics=False)
        for name, e in zip("abc", ens):
            v = e.verify(truth_member=0).scores
            print(f"cycle {cyc}: ({name}) rmse {v.rmse:.5f} spread {v.spread:.5f}")
        for e in ens:
            assert same_bits(e.download(0), truth)
    for e in ens:
        e.close()
