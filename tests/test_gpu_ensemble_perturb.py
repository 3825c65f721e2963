"""Ensemble perturbation (csim_ensemble_perturb) on the GPU against the numpy restatement of the block in
include/csim.h (tests/perturb_restatement.py, pinned to the library's host helpers and to independent references by
tests/test_ensemble_perturb_host.py), bit for bit; what it must leave alone; that a member's field is a pure function of
(seed, draw, member, cell); pipelining; the statistics of the fields; and an OSSE whose spread comes from perturb alone."""
import math

import numpy as np
import pytest

import perturb_restatement as ref
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
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def start_state(rng, B, ny, nx):
    X = rng.standard_normal((B, ny + 2, nx + 2))
    X[:, 1, 1] = -0.0  # a negative zero in the interior
    return X


# ---- the restatement ---------------------------------------------------------------------------------------------

# B, truth member, nx, ny, bc, dx, dy, corr_len, centered, sigma, seed, draw
CASES = [
    (2, None, 1, 1, "dddd", 1.0, 1.0, 0.0, 0, 0.5, 1, 0),
    (2, None, 1, 1, "pppp", 1.0, 1.0, 3.0, 1, 0.5, 1, 0),                    # periodic clip (n - 1) / 2 = 0
    (3, 0, 5, 1, "pppp", 1.0, 1.0, 4.0, 1, 1.5, (1 << 40) + 17, 3),         # odd Px, clip 2 and 0
    (3, 2, 5, 1, "dddd", 1.0, 1.0, 4.0, 0, -0.7, 99, 0),                    # clip n - 1 = 4, negative sigma
    (3, None, 2, 5, "nnnn", 1.0, 0.5, 0.4, 0, 0.3, 5, 1),                   # below one cell in x, Ry = 1
    (65, None, 2, 5, "ppdd", 0.7, 1.0, 2.0, 1, 0.1, 1 << 63, 2),            # periodic in x only, even Px
    (65, 64, 67, 130, "ddpp", 1.0, 0.8, 2.5, 0, 1.0, 12345678901234, 7),    # periodic in y only, tiles of 8 rows
    (3, 1, 67, 130, "pppp", 1.0, 1.0, 8.0, 1, 0.25, 3, 0xFFFFFFFF),         # R = 15, odd Px
    (9, 0, 130, 67, "nnnn", 1.0, 1.0, 16.2, 0, 2.0, 8, 1),                  # R = 32, the cap
    (320, 7, 12, 9, "dnpd", 1.0, 1.0, 1.2, 1, 0.6, (1 << 64) - 1, 5),       # a large ensemble
    (300, None, 12, 9, "pppp", 1.0, 1.0, 30.0, 0, 0.6, 4, 4),               # both periodic clips bind
    (65, 0, 300, 261, "dddd", 0.9, 1.1, 3.0, 0, 0.4, 77, 2),                # tiles of 32 rows, odd sizes
    (9, None, 512, 512, "pppp", 1.0, 1.0, 2.0, 0, 1.0, 2, 0),               # tiles of 32 rows, full tiles
    (3, 2, 512, 512, "dddd", 1.0, 1.0, 2.0, 1, 1.0, 2, 1),                  # centered, tiles of 8 rows
    (3, None, 1024, 520, "ddpp", 1.0, 1.0, 1.0, 1, 0.5, 21, 0),             # centered, tiles of 32 rows
]


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}_t{c[1]}_{c[2]}x{c[3]}_{c[4]}_c{c[7]}_cen{c[8]}" for c in CASES])
def test_restatement_bit_for_bit(csim, case):
    B, t, nx, ny, bcs, dx, dy, c, cen, sigma, seed, draw = case
    bc = csim.bc_codes(bcs)
    rng = np.random.default_rng(B * 1000 + nx)
    X = start_state(rng, B, ny, nx)
    e = csim.Ensemble(B, nx, ny, dx, dy, bc, 0.25)
    e.upload_all(X)
    e.perturb(sigma, c, seed, draw, centered=bool(cen), truth_member=t)
    got = e.download_all()
    e.close()
    want = ref.perturb(X, seed, draw, sigma, c, cen, t, dx, dy, bc)
    assert same_bits(got, want), f"{np.abs(got - want).max()}"
    # ghost ring and the truth member: the uploaded bits
    ring = np.ones((ny + 2, nx + 2), dtype=bool)
    ring[1:-1, 1:-1] = False
    assert same_bits(got[:, ring], X[:, ring])
    if t is not None:
        assert same_bits(got[t], X[t])
    assert not same_bits(got, X)


def test_sigma_zero_leaves_every_bit(csim):
    B, nx, ny = 4, 37, 21
    X = start_state(np.random.default_rng(0), B, ny, nx)
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
    e.upload_all(X)
    e.perturb(0.0, 2.0, 9)
    e.perturb(-0.0, 0.0, 9, centered=True)
    got = e.download_all()
    e.close()
    assert same_bits(got, X) and np.signbit(got[:, 1, 1]).all()


def test_argument_errors(csim):
    e = csim.Ensemble(3, 8, 8, 1.0, 1.0, (0, 0, 0, 0))
    one = csim.Ensemble(1, 8, 8, 1.0, 1.0, (0, 0, 0, 0))
    two = csim.Ensemble(2, 8, 8, 1.0, 1.0, (0, 0, 0, 0))
    big = csim.Ensemble(2, 200, 8, 1.0, 1.0, (0, 0, 0, 0))
    bad = [(e, dict(sigma=np.nan)), (e, dict(sigma=np.inf)), (e, dict(corr_len=-1.0)), (e, dict(corr_len=np.nan)),
           (e, dict(corr_len=np.inf)), (e, dict(centered=2)), (e, dict(centered=-1)), (e, dict(truth_member=3)),
           (e, dict(truth_member=-2)), (one, dict(truth_member=0)), (one, dict(centered=1)),
           (two, dict(centered=1, truth_member=1))]
    for ens, kw in bad:
        args = dict(sigma=1.0, corr_len=1.0, seed=1)
        args.update(kw)
        with pytest.raises(csim.CsimError) as ei:
            ens.perturb(**args)
        assert ei.value.code == 1, kw
    with pytest.raises(csim.CsimError) as ei:
        big.perturb(1.0, 16.6, 1)                     # Rx = 33
    assert ei.value.code == 5
    with pytest.raises(csim.CsimError) as ei:
        big.perturb(0.0, 16.6, 1)                     # refused even where nothing would be launched
    assert ei.value.code == 5
    one.perturb(1.0, 1.0, 1)                          # one forecast member is enough without centring
    two.perturb(1.0, 1.0, 1, centered=True)
    assert np.isfinite(e.download_all()).all() and np.abs(one.download(0)[1:-1, 1:-1]).min() > 0
    for ens in (e, one, two, big):
        ens.close()


# ---- a pure function of (seed, draw, member, cell) ------------------------------------------------------------------

def increment(csim, B, nx, ny, bc, seed, draw, c=2.0, **kw):
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, bc)
    e.perturb(1.0, c, seed, draw, **kw)   # on a zero state: 0 + 1.0 * p = p
    X = e.download_all()
    e.close()
    return X


def test_member_fields_do_not_depend_on_the_ensemble(csim):
    nx, ny, bc = 70, 45, csim.bc_codes("dnpd")
    a = increment(csim, 5, nx, ny, bc, 11, 2)
    b = increment(csim, 70, nx, ny, bc, 11, 2)                      # other member shares, other launch
    c = increment(csim, 5, nx, ny, bc, 11, 2, truth_member=1)
    assert same_bits(a, b[:5]) and same_bits(a, increment(csim, 5, nx, ny, bc, 11, 2))
    assert same_bits(c[[0, 2, 3, 4]], a[[0, 2, 3, 4]]) and not c[1].any()
    inner = (slice(None), slice(1, -1), slice(1, -1))
    for other in (increment(csim, 5, nx, ny, bc, 12, 2), increment(csim, 5, nx, ny, bc, 11, 3),
                  increment(csim, 5, nx, ny, bc, 11 + (1 << 32), 2)):
        assert (other[inner] != a[inner]).mean() > 0.999
    for k in range(1, 5):
        assert (a[k][1:-1, 1:-1] != a[0][1:-1, 1:-1]).mean() > 0.999


# ---- pipelining --------------------------------------------------------------------------------------------------

PHYS = [(0.05, 0.1, 0.5, -0.25), (0.02, 0.1, -0.3, 0.4), (0.08, 0.05, 0.0, 0.0), (0.01, 0.1, 0.2, 0.2)]


@pytest.mark.parametrize("bcs", ["dddd", "nnnn", "pppp"])
def test_run_perturb_run_matches_stepper(csim, bcs):
    bc = csim.bc_codes(bcs)
    B, nx, ny, n = 4, 70, 45, 9
    X = start_state(np.random.default_rng(3), B, ny, nx)
    phys = [[p[k] for p in PHYS] for k in range(4)]

    def make():
        e = csim.Ensemble(B, nx, ny, 1.0, 0.8, bc, 0.5)
        e.upload_all(X)
        e.set_physics(*phys)
        return e

    e = make()
    e.run(n)
    e.perturb(0.3, 2.0, 5, 1, truth_member=2)   # no sync in between
    e.run(n)
    got = e.download_all()
    e.close()
    # the same with a download after the perturbation, which a Stepper then continues
    e = make()
    e.run(n)
    before = e.download_all()
    e.perturb(0.3, 2.0, 5, 1, truth_member=2)
    mid = e.download_all()
    e.close()
    assert same_bits(mid, ref.perturb(before, 5, 1, 0.3, 2.0, 0, 2, 1.0, 0.8, bc))
    for m in range(B):
        st = csim.Stepper.single(nx, ny, 1.0, 0.8, bc, 0.5)
        st.upload(mid[m])
        st.run(*PHYS[m], n)
        want = st.download()
        st.close()
        assert same_bits(got[m], want), f"member {m}, {bcs}"
    # The buffer that is not current cannot be downloaded.  What a later run reads of it is its ghost ring, which
    # periodic sides keep for good: the comparison above, an odd number of buffer swaps after the perturbation, fails
    # for "pppp" if the perturbation had written there.


def test_assimilate_perturb_run_pipelines_and_captures_see_the_state_before(csim):
    B, nx, ny = 12, 96, 64
    rng = np.random.default_rng(11)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j = rng.integers(1, nx + 1, 60), rng.integers(1, ny + 1, 60)
    y = rng.standard_normal(60)
    runs = []
    for sync in (False, True):
        e = csim.Ensemble(B, nx, ny, 1.0, 1.0, csim.bc_codes("dnpd"))
        e.upload_all(X)
        e.set_physics(0.05, 0.1, 0.5, -0.25)
        e.run(4)
        s0 = e.stats()
        e.assimilate(i, j, y, 0.5, 4.0, inflation=1.02, truth_member=0, diagnostics=False)
        if sync:
            e.sync()
        s1 = e.stats() if sync else None
        e.stats_begin()
        e.perturb(0.2, 3.0, 8, 1, centered=True, truth_member=0)
        if sync:
            e.sync()
        e.run(7)
        runs.append(e.download_all())
        cap = e.stats_wait()
        if sync:
            assert same_bits(cap.mean, s1.mean) and same_bits(cap.var, s1.var)
            assert not same_bits(cap.var, s0.var)
        e.close()
    assert same_bits(runs[0], runs[1])


# ---- statistics --------------------------------------------------------------------------------------------------

def test_field_statistics(csim):
    """64 members of 512 x 512 on a bounded grid: N = 64 * 512^2 = 1.68e7 samples of p.  Neighbouring samples are
    correlated over 2 R + 1 cells per axis, so N_eff = N / (2 R + 1)^2 independent samples is a safe undercount.
    For unit-variance Gaussians the sample mean has standard deviation 1 / sqrt(N_eff), and the sample mean of a
    product of two of them (variance, lagged covariance) at most sqrt(2 / N_eff); the bounds are six of those."""
    B, n, c = 64, 512, 2.0
    P = increment(csim, B, n, n, (0, 0, 0, 0), 2024, 0, c=c)[:, 1:-1, 1:-1]
    t = ref.taps(1.0, c, n, False)
    R = len(t) // 2
    assert R == 3
    n_eff = P.size / (2 * R + 1) ** 2
    mean_bound, prod_bound = 6 / math.sqrt(n_eff), 6 * math.sqrt(2 / n_eff)
    print(f"mean {P.mean():.3e} (bound {mean_bound:.3e}), var {P.var():.6f} (1 +- {prod_bound:.3e})")
    assert abs(P.mean()) <= mean_bound
    assert abs(np.mean(P * P) - 1.0) <= prod_bound
    # unit variance up to the edge: the outermost ring of cells, 64 * 2044 samples, N_eff again divided by 2 R + 1
    # along the edge only
    edge = np.concatenate([P[:, 0, :].ravel(), P[:, -1, :].ravel(), P[:, 1:-1, 0].ravel(), P[:, 1:-1, -1].ravel()])
    assert abs(np.mean(edge * edge) - 1.0) <= 6 * math.sqrt(2 * (2 * R + 1) / edge.size)
    for lag in range(1, 2 * R + 2):
        want = float(np.sum(t[:len(t) - lag] * t[lag:])) if lag <= 2 * R else 0.0
        ax = np.mean(P[:, :, :-lag] * P[:, :, lag:])
        ay = np.mean(P[:, :-lag, :] * P[:, lag:, :])
        print(f"lag {lag}: x {ax:.5f}, y {ay:.5f}, want {want:.5f}")
        assert abs(ax - want) <= prod_bound and abs(ay - want) <= prod_bound


def test_centered_increments_have_zero_mean(csim):
    """On a zero state with sigma = 0.5 the update 0 + 0.5 (p_k - pbar) is exact, so the per-cell mean of the
    increments is 0.5 / M times the sum of the rounded p_k - pbar.  With u = 2^-53: the running sum of the p_k errs by
    at most (M - 1) u max|partial sum|, the division by M adds u |pbar|, each difference u |p_k - pbar|; so
    |mean| <= 0.5 u (max|partial sum| + |pbar| + max|p_k - pbar|) — a few ulp of sigma.  The mean itself is
    formed exactly (math.fsum)."""
    B, nx, ny, bc = 64, 40, 24, (0, 0, 0, 0)
    P = increment(csim, B, nx, ny, bc, 5, 0)[:, 1:-1, 1:-1]
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, bc)
    e.perturb(0.5, 2.0, 5, 0, centered=True)
    Q = e.download_all()[:, 1:-1, 1:-1]
    e.close()
    pbar = np.cumsum(P, axis=0)[-1] / B
    bound = 0.5 * 2.0 ** -53 * (np.abs(np.cumsum(P, axis=0)).max(axis=0) + np.abs(pbar) + np.abs(P - pbar).max(axis=0))
    mean = np.array([[math.fsum(Q[:, j, i]) / B for i in range(nx)] for j in range(ny)])
    print(f"largest |mean increment| {np.abs(mean).max():.3e}, largest bound {bound.max():.3e}")
    assert (np.abs(mean) <= bound).all()
    assert same_bits(Q, 0.5 * (P - pbar))


# ---- an OSSE whose spread comes from perturb alone -----------------------------------------------------------------

def test_osse_cycles_without_an_upload(csim):
    """Truth (member 0) and forecast members start as the same hotspot plus one draw each of the same noise, so the
    ensemble is statistically consistent with its error.  Cycles of run -> assimilate -> perturb (centred additive
    noise) against a free run from the same bits: the analysis mean stays closer to the truth than the free mean, and
    the spread stays above the noise just added: each centred draw adds sigma_add^2 (M - 1) / M of variance that is
    independent of the state, so 0.7 sigma_add is a safe floor for the spread."""
    B, nx, ny, sigma0, sigma_add, corr = 33, 96, 96, 0.05, 0.01, 5.0
    ens = []
    for _ in range(2):
        e = csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0))
        for m in range(B):
            e.init_gaussian(m, 1.0, 0.08, 0.5, 0.5)
        e.set_physics(0.05, 0.1, 0.3, 0.1)
        e.perturb(sigma0, corr, 2025, 0)
        ens.append(e)
    cyc, free = ens
    g = np.arange(2, nx + 1, 4)
    I, J = np.meshgrid(g, g)
    i, j = I.ravel(), J.ravel()
    rng = np.random.default_rng(4)
    r_obs = 0.005
    for c in range(1, 5):
        cyc.run(5), free.run(5)
        truth = cyc.download(0)
        assert same_bits(truth, free.download(0))
        y = truth[j, i] + r_obs * rng.standard_normal(len(i))
        cyc.assimilate(i, j, y, r_obs * r_obs, corr, truth_member=0, diagnostics=False)
        va, vf = cyc.verify(truth_member=0), free.verify(truth_member=0)
        print(f"cycle {c}: analysis rmse {va.scores.rmse:.5f} spread {va.scores.spread:.5f}, "
              f"free rmse {vf.scores.rmse:.5f} spread {vf.scores.spread:.5f}")
        assert va.scores.rmse < vf.scores.rmse
        cyc.perturb(sigma_add, corr, 2025, c, centered=True, truth_member=0)
        assert cyc.verify(truth_member=0).scores.spread >= 0.7 * sigma_add
        assert same_bits(cyc.download(0), truth)
    cyc.close(), free.close()
