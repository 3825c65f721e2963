"""The per-cell sorting kernels (csim_ensemble_quantiles*, csim_ensemble_verify*) at their network, tile and layout
seams.  The cases come from tests/order_stat_cases.py (what they reach is checked on the CPU by
tests/test_order_stat_cases_host.py): every lane and wave network empty-but-one, full and one past full, both sides of
every switch of the tile size, the loader's trip edges; 0/1 inputs (exhaustive up to 16 values, by count of ones above)
and structured permutations instead of random normals; and levels k / (M - 1) that read every sorted position, so that
the quantile kernels' own copies of the networks are seen whole.  The references are the existing ones, bit for bit:
np.quantile / np.mean for the quantiles and exceedances (assert_quantiles' rules), the numpy restatement of
include/csim.h for the verification (check_all), np.mean / np.var / fmin / fmax for the statistics that share the
dense layout.

The largest upload is the 4096-member counted case: order_stat_cases.CELL_CAP keeps a packed grid to 4096 cells, 134 MB
of members at most (it uses about 500 cells, 16 MB)."""
import os

import numpy as np
import pytest

import order_stat_cases as osc
from test_gpu_ensemble import csim, random_fields  # noqa: F401 (fixture)
from test_gpu_ensemble_quantiles import LEVELS, assert_quantiles, ensemble_with, nasty_members
from test_gpu_ensemble_stats import assert_stats
from test_gpu_ensemble_verify import THR, check_all, pairwise_crps, same_scores

pytestmark = pytest.mark.gpu


def assert_all_positions(e, a, what, ts=(0.0, 0.5)):
    """e.quantiles at the levels k / (B - 1), k = 0..B-1, sixteen per call, by assert_quantiles' rules: equal with NaN
    by position everywhere, by integer view wherever numpy's value is neither zero nor NaN.  The first call, which
    carries the thresholds, against np.quantile itself; all of them against np.quantile as one np.sort gives it
    (order_stat_cases.sorted_quantiles, held to np.quantile on the CPU)"""
    calls = osc.all_positions_levels(a.shape[0])
    want = osc.sorted_quantiles(a, np.concatenate(calls))
    k0 = 0
    for n, qs in enumerate(calls):
        got = e.quantiles(qs, ts if n == 0 else ())
        if n == 0:
            assert_quantiles(got, a, qs, list(ts), what)
        w = want[k0:k0 + len(qs)]
        assert got.q.shape == w.shape, what
        assert np.array_equal(got.q, w, equal_nan=True), f"{what}: positions {k0}..{k0 + len(qs) - 1}"
        exact = (w != 0) & ~np.isnan(w)
        assert np.array_equal(got.q[exact].view(np.int64), w[exact].view(np.int64)), \
            f"{what}: positions {k0}..{k0 + len(qs) - 1}, bits"
        k0 += len(qs)


def verify_both(e, x, y, what, truth_member=None, pairwise_cells=0):
    """check_all for both normalisations (fair needs two forecast members), with a host truth y or a truth member;
    the CRPS of the first `pairwise_cells` cells of row 0 also against its pairwise definition"""
    M = x.shape[0]
    for fair in ([False, True] if M >= 2 else [False]):
        kw = dict(truth_member=truth_member) if truth_member is not None else dict(truth=y)
        got = e.verify(**kw, thresholds=THR, fair=fair)
        crps, _ = check_all(got, x, y, THR, fair, f"{what}, fair = {fair}")
        if pairwise_cells:
            sl = (slice(0, 1), slice(0, pairwise_cells))
            want = pairwise_crps(x[(slice(None),) + sl], y[sl], fair)
            assert np.allclose(crps[sl], want, rtol=1e-12, atol=1e-13), f"{what}: pairwise definition"


def truth_with_ties(a, rng, zero_one):
    """a truth per cell: from {0, 0.5, 1} for 0/1 members; otherwise a normal deviate, in a quarter of the cells one
    of the cell's own members (a tie)"""
    shape = a.shape[1:]
    if zero_one:
        return rng.choice([0.0, 0.5, 1.0], shape)
    y = rng.standard_normal(shape)
    own = np.take_along_axis(a, rng.integers(0, a.shape[0], (1,) + shape), axis=0)[0]
    return np.where((rng.random(shape) < 0.25) & np.isfinite(own), own, y)


# ---- (a) every 0/1 input of the networks up to 16 values -----------------------------------------------------------

@pytest.mark.parametrize("M", range(1, 17))
def test_zero_one_exhaustive(csim, M):
    a = osc.zero_one_exhaustive(M)
    e = ensemble_with(csim, a)
    assert_all_positions(e, a, f"every 0/1 input of {M} values")   # M <= 16: the whole sorted column in one call
    y = truth_with_ties(a, np.random.default_rng(M), True)
    verify_both(e, a, y, f"every 0/1 input of {M} values")
    e.close()


# ---- (b) counted 0/1 inputs and structured permutations at every member-count seam -----------------------------------

def seam_members(B):
    """(members, zero_one mask per dense cell, cells of row 0 with distinct finite members)"""
    cols, _, n_distinct = osc.structured(B)
    counted = osc.zero_one_counts(B, 4 if B <= 64 else 2 if B <= 256 else 1)
    a = osc.pack(np.concatenate([cols, counted], axis=1))
    flat = np.arange(a.shape[1] * a.shape[2]) % (cols.shape[1] + counted.shape[1])
    # (the pairwise definition costs B^2 per cell: eight cells of distinct values, two above 1024 members)
    return a, (flat >= cols.shape[1]).reshape(a.shape[1:]), min(n_distinct, 8 if B <= 1024 else 2)


@pytest.mark.parametrize("B", osc.MEMBER_SEAMS)
def test_member_seams_counted_and_structured(csim, B):
    a, zero_one, distinct = seam_members(B)
    e = ensemble_with(csim, a)
    assert_all_positions(e, a, f"B = {B}")
    rng = np.random.default_rng(B)
    y = np.where(zero_one, truth_with_ties(a, rng, True), truth_with_ties(a, rng, False))
    verify_both(e, a, y, f"B = {B}, host truth", pairwise_cells=distinct)
    if B >= 2:
        t = (7 * B) // 11
        verify_both(e, np.delete(a, t, axis=0), a[t], f"B = {B}, truth member {t}", truth_member=t,
                    pairwise_cells=distinct)
    e.close()


# ---- (c) the truth member on a lane boundary of a full wave network --------------------------------------------------

@pytest.mark.parametrize("B,t", [(B, t) for B in osc.TRUTH_LANE_MEMBERS for t in (0, 63, 64, 65, B - 1)])
def test_truth_member_on_a_lane_boundary(csim, B, t):
    a = random_fields(B, 13, 5, seed=B + t)
    others = np.delete(a, t, axis=0)
    e, rest = ensemble_with(csim, a), ensemble_with(csim, others)
    for fair in (False, True):
        got = e.verify(truth_member=t, thresholds=THR, fair=fair)
        ref = rest.verify(e.download(t), thresholds=THR, fair=fair)
        for f in ("crps", "brier", "rank_hist"):
            assert np.array_equal(getattr(got, f).view(np.int64), getattr(ref, f).view(np.int64)), f
        assert same_scores(got.scores, ref.scores)
        check_all(got, others, a[t], THR, fair, f"B = {B}, t = {t}, fair = {fair}")
    e.close()
    rest.close()


# ---- (d) the dense layout on its row seams ---------------------------------------------------------------------------

def layout_check(csim, nx, ny, B):
    seed = 1000 * B + nx + ny
    if ny >= 2:
        a = nasty_members(B, nx, ny, seed)
    else:   # its special cells need four rows: laid out along the other axis
        a = np.ascontiguousarray(nasty_members(B, ny, nx, seed).transpose(0, 2, 1))
    e = ensemble_with(csim, a)
    what = f"{B} x {nx}x{ny}"
    for ddof in (0, 1):
        assert_stats(e.stats(ddof), a, ddof, what)
    assert_quantiles(e.quantiles(LEVELS, (0.0, 0.5)), a, LEVELS, [0.0, 0.5], what)
    rng = np.random.default_rng(B + nx)
    y = rng.standard_normal((ny + 2, nx + 2))
    y[rng.random(y.shape) < 0.01] = np.nan
    y[-1, -1] = 0.5   # the last dense cell, which the lanes past the end load again
    verify_both(e, a, y, what)
    t = B // 2
    verify_both(e, np.delete(a, t, axis=0), a[t], f"{what}, truth member {t}", truth_member=t)
    e.close()


@pytest.mark.parametrize("B", [12, 70, 100])
@pytest.mark.parametrize("shape", osc.LAYOUT_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in osc.LAYOUT_SHAPES])
def test_layout_seams(csim, shape, B):
    layout_check(csim, *shape, B)


@pytest.mark.parametrize("shape", osc.GRID_MAX_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in osc.GRID_MAX_SHAPES])
def test_layout_at_the_verification_grid_limit(csim, shape):
    """the lane form's launch of exactly VERIFY_GRID_MAX workgroups, and the first grid on which one of them loops"""
    layout_check(csim, *shape, 12)


# ---- (e) random data at every wave-form seam, every position read --------------------------------------------------

@pytest.mark.parametrize("B", [B for B in osc.MEMBER_SEAMS if B > 64])
def test_random_soak(csim, B):
    seed = int(os.environ.get("CSIM_ORDER_STAT_SEED", osc.DEFAULT_SEED))   # (other seeds: extended soak runs)
    rng = np.random.default_rng([seed, B])
    nx, ny = int(rng.integers(1, 12)), int(rng.integers(1, 8))
    a = rng.standard_normal((B, ny + 2, nx + 2))
    a[rng.integers(B), 0, 0] = np.nan                      # one NaN member in one cell
    a[: rng.integers(1, B), 0, 1] = a[0, 0, 1]             # a run of ties
    e = ensemble_with(csim, a)
    what = f"seed {seed}, {B} x {nx}x{ny}"
    assert_all_positions(e, a, what, ts=(0.0, float(a[B // 2, 1, 1])))
    verify_both(e, a, truth_with_ties(a, rng, False), what)
    t = int(rng.integers(B))
    verify_both(e, np.delete(a, t, axis=0), a[t], f"{what}, truth member {t}", truth_member=t)
    e.close()
