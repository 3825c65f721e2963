"""Neighbourhood and probability verification on the GPU (csim_ensemble_verify_spatial*): every integer output against
the numpy restatement of tests/spatial_restatement.py with ==, the finished scores bit for bit, at the seams of both
kernels (tile sides, the member split, the grid caps), with ties, infinities and NaN, as a capture, and against what
the package already computes (quantiles' exceedance probabilities, verify's Brier scores)."""
import math

import numpy as np
import pytest

import spatial_restatement as ref
from __graft_entry__ import load_package
from test_gpu_ensemble import PHYS12, random_fields

pytestmark = pytest.mark.gpu

TILE = 32                                   # SPATIAL_TILE of ensemble.hpp: centres per tile side of the score pass
HALVES = (0, 1, 2, 4, 8, 16, 32)
THR = [0.0, 0.5, -1.0]
SHAPES = [(1, 1), (5, 3), (64, 64), (65, 33), (67, 48), (130, 70),
          (TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1)]
SMALL = [(1, 1), (5, 3), (TILE + 1, TILE - 1), (64, 64)]
CASES = [(s, M) for s in SHAPES for M in (1, 2, 5, 63, 64, 65)] + [(s, 130) for s in SMALL] + \
        [(s, 1000) for s in SMALL[:3]]


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def ensemble_with(csim, u0s):
    B, ny2, nx2 = u0s.shape
    e = csim.Ensemble(B, nx2 - 2, ny2 - 2, 1.0, 1.0, (0, 0, 0, 0))
    e.upload_all(u0s)
    return e


def flags_of(r):
    fl = np.zeros(r["nan"].shape, dtype=np.uint32)
    for q in range(r["o"].shape[0]):
        fl |= (r["o"][q].astype(np.uint32) << np.uint32(q))
    fl[r["nan"]] = np.uint32(1 << 31)
    return fl


def check(got, x, y, thr, halves, what):
    """got: SpatialVerification with counts; x: the forecast members, y: the truth"""
    M = len(x)
    r = ref.restate(x, y, thr, halves)
    assert (got.cells, got.nan_cells) == (r["cells"], r["nan_cells"]), what
    assert got.table.dtype == np.uint64 and got.table.shape == (len(thr), M + 1, 2), what
    assert np.array_equal(got.table, r["table"]), what
    assert got.nbh.shape == (len(thr), len(halves), 3) and np.array_equal(got.nbh, r["nbh"]), what
    if got.counts is not None:
        assert got.counts.dtype == np.uint16 and np.array_equal(got.counts, r["n"]), what
        assert got.flags.dtype == np.uint32 and np.array_equal(got.flags, flags_of(r)), what
    assert ref.scores_match(got.scores, r["scores"]) == [], what
    return r


def same_result(a, b):
    return (a.cells, a.nan_cells) == (b.cells, b.nan_cells) and np.array_equal(a.table, b.table) and \
        np.array_equal(a.nbh, b.nbh) and np.array_equal(a.counts, b.counts) and np.array_equal(a.flags, b.flags) and \
        all(ref.same_bits(getattr(a.scores, k), getattr(b.scores, k)) for k in a.scores._fields[2:])


# ---- shapes, members, truths ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,M", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_against_the_restatement(csim, shape, M):
    nx, ny = shape
    u = random_fields(M + 2, nx, ny, seed=1000 * nx + 10 * ny + M)
    # a host truth against M members
    e = ensemble_with(csim, np.ascontiguousarray(u[:M]))
    check(e.verify_spatial(u[M + 1], thresholds=THR, half_widths=HALVES, counts=True), u[:M], u[M + 1], THR, HALVES,
          f"{shape} M={M} host truth")
    e.close()
    # member 0, a middle member, the last member against the M others
    e = ensemble_with(csim, np.ascontiguousarray(u[:M + 1]))
    for t in sorted({0, (M + 1) // 2, M}):
        x = np.delete(u[:M + 1], t, axis=0)
        check(e.verify_spatial(truth_member=t, thresholds=THR, half_widths=HALVES, counts=True), x, u[t], THR, HALVES,
              f"{shape} M={M} truth member {t}")
    e.close()


def test_half_width_lists_and_threshold_counts(csim):
    nx, ny, M = 67, 48, 5
    u = random_fields(M + 1, nx, ny, seed=3)
    e = ensemble_with(csim, np.ascontiguousarray(u[:M]))
    base = check(e.verify_spatial(u[M], thresholds=THR, half_widths=HALVES), u[:M], u[M], THR, HALVES, "ordered")
    scrambled = (8, 0, 32, 2, 8, 16, 1, 4)  # any order, a repeat, all eight scales
    got = e.verify_spatial(u[M], thresholds=THR, half_widths=scrambled, counts=True)
    check(got, u[:M], u[M], THR, scrambled, "scrambled")
    for s, h in enumerate(scrambled):
        assert np.array_equal(got.nbh[:, s], base["nbh"][:, HALVES.index(h)])
    assert np.array_equal(got.nbh[:, 0], got.nbh[:, 4])
    none = e.verify_spatial(u[M], thresholds=THR)  # ns = 0
    check(none, u[:M], u[M], THR, (), "no scales")
    assert none.nbh.shape == (3, 0, 3) and none.scores.fss.shape == (3, 0) and none.counts is None
    check(e.verify_spatial(u[M], thresholds=[0.25], half_widths=(3,), counts=True), u[:M], u[M], [0.25], (3,), "nt = 1")
    thr16 = [float(v) for v in np.linspace(-2.0, 2.0, 16)]
    check(e.verify_spatial(u[M], thresholds=thr16, half_widths=(0, 5, 32), counts=True), u[:M], u[M], thr16, (0, 5, 32),
          "nt = 16")
    e.close()


# ---- launch seams --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,M", [((64, 64), 130), ((5, 3), 1000), ((65, 33), 5), ((33, 31), 257)],
                         ids=["64x64-130", "5x3-1000", "65x33-5", "33x31-257"])
def test_member_split_equals_unsplit(csim, shape, M):
    """the default split of the count pass (3 parts at 64 x 64 with 130 members, 16 at 5 x 3 with 1000, none with 5)
    and forced splits against one part, on the same data; a NaN in one part must still mark the cell"""
    nx, ny = shape
    u = random_fields(M + 1, nx, ny, seed=M)
    u[M - 1, ny, nx] = np.nan      # the last member: the last part
    u[0, 1, 1] = np.inf
    e = ensemble_with(csim, u)
    x = np.delete(u, 1, axis=0)
    assert e.get_option("spatial_member_split") == 0
    auto = e.verify_spatial(truth_member=1, thresholds=THR, half_widths=(0, 3), counts=True)
    check(auto, x, u[1], THR, (0, 3), "default split")
    for parts in (1, 2, 7, M, 4096):
        e.set_option("spatial_member_split", parts)
        assert e.get_option("spatial_member_split") == parts
        got = e.verify_spatial(truth_member=1, thresholds=THR, half_widths=(0, 3), counts=True)
        assert same_result(got, auto), parts
    e.close()


def test_grid_caps_do_not_change_the_result(csim):
    nx, ny, M = 130, 70, 5
    u = random_fields(M + 1, nx, ny, seed=11)
    u[2, 40, 100] = np.nan
    e = ensemble_with(csim, u)
    x = np.delete(u, M, axis=0)
    assert e.get_option("spatial_grid_max") == 0
    want = e.verify_spatial(truth_member=M, thresholds=THR, half_widths=HALVES, counts=True)
    check(want, x, u[M], THR, HALVES, "default caps")
    for cap in (1, 2, 3):
        e.set_option("spatial_grid_max", cap)
        assert e.get_option("spatial_grid_max") == cap
        assert same_result(e.verify_spatial(truth_member=M, thresholds=THR, half_widths=HALVES, counts=True), want), cap
    e.set_option("spatial_member_split", 3)  # the split pass under the cap as well
    assert same_result(e.verify_spatial(truth_member=M, thresholds=THR, half_widths=HALVES, counts=True), want)
    for key in ("spatial_grid_max", "spatial_member_split"):
        with pytest.raises(csim.CsimError):
            e.set_option(key, -1)
        with pytest.raises(csim.CsimError):
            e.set_option(key, 70000)
    e.close()


# ---- ties and special values ---------------------------------------------------------------------------------------

def test_ties_zeros_and_infinities(csim):
    nx, ny, M = 65, 33, 6
    rng = np.random.default_rng(21)
    vals = np.array([-1.0, -0.0, 0.0, 1.0, 2.0])
    u = vals[rng.integers(0, 5, size=(M + 1, ny + 2, nx + 2))]
    thr = [-0.0, 0.0, 1.0, 2.0, np.inf, -np.inf]
    e = ensemble_with(csim, u)
    x = np.delete(u, 0, axis=0)
    got = e.verify_spatial(truth_member=0, thresholds=thr, half_widths=(0, 1, 7), counts=True)
    check(got, x, u[0], thr, (0, 1, 7), "ties")
    assert np.array_equal(got.counts[0], got.counts[1])          # -0.0 and 0.0 are one threshold
    assert not got.counts[4].any() and np.all(got.counts[5] == M)  # nothing exceeds +Inf, every finite value -Inf
    assert got.table[3, :, 1].sum() == 0                         # the truth never exceeds its own maximum
    # infinite members and an infinite truth
    u[1, 5, 5], u[2, 5, 5], u[3, 6, 6], u[0, 7, 7], u[0, 8, 8] = np.inf, np.inf, -np.inf, np.inf, -np.inf
    e.upload_all(u)
    x = np.delete(u, 0, axis=0)
    got = e.verify_spatial(truth_member=0, thresholds=thr, half_widths=(0, 1, 7), counts=True)
    check(got, x, u[0], thr, (0, 1, 7), "infinities")
    assert got.counts[4].sum() == 0 and got.counts[5, 5, 5] == M - 1  # -Inf does not exceed -Inf
    assert got.flags[6, 6] >> 4 & 1 == 0 and got.flags[6, 6] >> 3 & 1 == 1 and got.flags[7, 7] >> 5 & 1 == 0
    assert got.nan_cells == 0
    e.close()


def nan_places(nx, ny):
    """interior (j, i) index lists, 1-based as in the field: a corner, both sides of a tile seam, a whole row"""
    return {"corner": [(1, 1)], "far_corner": [(ny, nx)], "seam": [(TILE, TILE), (TILE + 1, TILE + 1), (TILE, TILE + 1)],
            "row": [(TILE + 1, i) for i in range(1, nx + 1)]}


@pytest.mark.parametrize("where", ["corner", "far_corner", "seam", "row"])
@pytest.mark.parametrize("who", ["truth", "member"])
def test_nan_cells(csim, where, who):
    nx, ny, M = 67, 48, 5
    u = random_fields(M + 1, nx, ny, seed=31)
    u[:, 0, :] = np.nan  # the ghost ring is never read as data
    u[:, :, -1] = np.nan
    k = M if who == "truth" else 2
    for (j, i) in nan_places(nx, ny)[where]:
        u[k, j, i] = np.nan
    e = ensemble_with(csim, np.ascontiguousarray(u[:M]))
    got = e.verify_spatial(u[M], thresholds=THR, half_widths=HALVES, counts=True)
    r = check(got, u[:M], u[M], THR, HALVES, f"NaN {who} {where}")
    n = len(nan_places(nx, ny)[where])
    assert got.nan_cells == n and got.cells == nx * ny - n == r["cells"]
    assert np.count_nonzero(got.flags >> 31) == n and not got.counts[:, got.flags >> 31 != 0].any()
    e.close()


def test_all_cells_nan(csim):
    nx, ny, M = 33, 31, 3
    u = random_fields(M + 1, nx, ny, seed=41)
    u[1] = np.nan
    e = ensemble_with(csim, np.ascontiguousarray(u[:M]))
    got = e.verify_spatial(u[M], thresholds=THR, half_widths=(0, 4), counts=True)
    check(got, u[:M], u[M], THR, (0, 4), "all NaN")
    assert got.cells == 0 and got.nan_cells == nx * ny and not got.table.any() and not got.nbh.any()
    s = got.scores
    for v in (s.brier, s.reliability, s.resolution, s.uncertainty, s.roc_area, s.fss, s.hit_rate, s.false_alarm):
        assert np.all(np.isnan(v))
    e.close()


# ---- the case with teeth -------------------------------------------------------------------------------------------

def bump(nx, ny, ci, cj):
    f = np.zeros((ny + 2, nx + 2))
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    f[1:-1, 1:-1] = np.exp(-((ii - ci) ** 2 + (jj - cj) ** 2) / 18.0)
    return f


def test_displaced_hotspot_gains_skill_with_scale(csim):
    nx, ny, M = 67, 48, 5
    truth = bump(nx, ny, 30, 24)
    x = np.array([bump(nx, ny, 36 + k, 23 + k % 3) for k in range(M)])
    e = ensemble_with(csim, x)
    got = e.verify_spatial(truth, thresholds=[0.5], half_widths=HALVES, counts=True)
    check(got, x, truth, [0.5], HALVES, "displaced hotspot")
    fss = got.scores.fss[0]
    assert np.allclose(fss, [0.0131, 0.0340, 0.0751, 0.2517, 0.6092, 0.8123, 0.9376], rtol=0, atol=5e-5), fss
    assert np.all(np.diff(fss) > 0)
    assert fss[HALVES.index(4)] < 0.5 < fss[HALVES.index(8)]
    # the double penalty at grid scale: the displaced forecast scores worse than a forecast of nothing
    grid = e.verify(truth, thresholds=[0.5]).scores.brier[0]
    e.close()
    empty = ensemble_with(csim, np.zeros_like(x))
    nothing = empty.verify(truth, thresholds=[0.5]).scores.brier[0]
    none = empty.verify_spatial(truth, thresholds=[0.5], half_widths=HALVES)
    empty.close()
    assert grid > nothing > 0.0
    # the table's Brier score is verify()'s mean of the same 3216 terms in another order
    assert abs(got.scores.brier[0] - grid) <= 1e-12 and abs(none.scores.brier[0] - nothing) <= 1e-12
    assert np.all(none.scores.fss[0] == 0.0)


# ---- against what already ships ------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [5, 65])
def test_against_quantiles_and_verify(csim, M):
    nx, ny = 65, 33
    u = random_fields(M + 1, nx, ny, seed=50 + M)
    e = ensemble_with(csim, np.ascontiguousarray(u[:M]))
    got = e.verify_spatial(u[M], thresholds=THR, counts=True)
    p = e.quantiles((), THR).exceed[:, 1:-1, 1:-1]
    assert ref.same_bits(got.counts.astype(np.float64) / float(M), p)
    brier = e.verify(u[M], thresholds=THR).brier[:, 1:-1, 1:-1]
    for q in range(len(THR)):
        assert math.fsum(brier[q].ravel().tolist()) == ref.fsum_brier_terms(got.table[q], M), q
    e.close()


# ---- captures ------------------------------------------------------------------------------------------------------

def test_begin_run_wait_returns_the_state_before_the_run(csim):
    nx, ny, B = 67, 48, 6
    u = random_fields(B, nx, ny, seed=61)
    e = ensemble_with(csim, u)
    e.set_physics(*[[p[k] for p in PHYS12[:B]] for k in range(4)])
    sums = e.checksums()
    e.verify_spatial_begin(truth_member=2, thresholds=THR, half_widths=HALVES, counts=True)
    assert e.checksums() == sums  # the call writes no member
    assert np.array_equal(e.download_all()[:, 1:-1, 1:-1], u[:, 1:-1, 1:-1])
    e.run(5)
    got = e.verify_spatial_wait()
    check(got, np.delete(u, 2, axis=0), u[2], THR, HALVES, "begin; run(5); wait")
    with pytest.raises(csim.CsimError) as err:
        e.verify_spatial_wait()
    assert err.value.code == 4
    # a host truth is copied before _begin returns; without fields only the tables come back
    now = e.download_all()
    truth = random_fields(1, nx, ny, seed=62)[0]
    mine = truth.copy()
    e.verify_spatial_begin(mine, thresholds=THR, half_widths=(2, 9))
    mine[:] = np.nan
    e.run(3)
    e.verify_spatial(truth_member=0, thresholds=[0.1])  # a synchronous call leaves the capture alone
    got = e.verify_spatial_wait()
    assert got.counts is None and got.flags is None
    check(got, now, truth, THR, (2, 9), "host truth; run; wait")
    e.close()


@pytest.mark.parametrize("order", ["spatial_first", "spatial_last"])
def test_in_flight_with_the_other_captures(csim, order):
    nx, ny, B = 65, 33, 5
    u = random_fields(B, nx, ny, seed=71)
    e = ensemble_with(csim, u)
    e.set_physics(*[[p[k] for p in PHYS12[:B]] for k in range(4)])
    others = [lambda: e.verify_begin(truth_member=1, thresholds=THR), lambda: e.stats_begin(1),
              lambda: e.quantiles_begin([0.5], [0.0])]
    mine = [lambda: e.verify_spatial_begin(truth_member=1, thresholds=THR, half_widths=(0, 4, 32), counts=True)]
    for call in (mine + others if order == "spatial_first" else others + mine):
        call()
    e.run(4)
    want = (e.verify(truth_member=1, thresholds=THR), e.stats(1), e.quantiles([0.5], [0.0]))  # of the state after the run
    if order == "spatial_first":
        got, v, st, qu = e.verify_spatial_wait(), e.verify_wait(), e.stats_wait(), e.quantiles_wait()
    else:
        v, st, qu, got = e.verify_wait(), e.stats_wait(), e.quantiles_wait(), e.verify_spatial_wait()
    check(got, np.delete(u, 1, axis=0), u[1], THR, (0, 4, 32), order)
    e2 = ensemble_with(csim, u)  # the other captures hold the state before the run as well
    assert ref.same_bits(v.crps, e2.verify(truth_member=1, thresholds=THR).crps)
    assert ref.same_bits(st.mean, e2.stats(1).mean) and ref.same_bits(qu.q, e2.quantiles([0.5], [0.0]).q)
    assert not ref.same_bits(st.mean, want[1].mean)
    e2.close()
    e.close()


# ---- errors --------------------------------------------------------------------------------------------------------

def test_errors(csim):
    lib, C = csim.lib(), csim.C
    nx, ny, B = 9, 7, 4
    e = ensemble_with(csim, random_fields(B, nx, ny, seed=81))
    truth = np.zeros((ny + 2, nx + 2))
    tp = truth.ctypes.data_as(C.POINTER(C.c_double))
    thr = (C.c_double * 17)(*([0.5] * 17))
    half = (C.c_int * 9)(*([1] * 9))

    def sync(t, tm, nt, th, ns, hw):
        return lib.csim_ensemble_verify_spatial(e._h, t, tm, nt, th, ns, hw, None, None, None, None, None, None)

    def begin(t, tm, nt, th, ns, hw, fields=0):
        return lib.csim_ensemble_verify_spatial_begin(e._h, t, tm, nt, th, ns, hw, fields)

    bad_half = [(C.c_int * 2)(1, -1), (C.c_int * 2)(33, 1)]
    for call in (sync, begin):
        assert call(None, -1, 1, thr, 0, None) == 1            # no truth
        assert call(tp, 0, 1, thr, 0, None) == 1               # two truths
        assert call(None, B, 1, thr, 0, None) == 1             # truth_member outside -1 .. B-1
        assert call(None, -2, 1, thr, 0, None) == 1
        assert call(tp, -1, 0, thr, 0, None) == 1              # nt outside 1 .. 16
        assert call(tp, -1, 17, thr, 0, None) == 1
        assert call(tp, -1, 1, None, 0, None) == 1
        assert call(tp, -1, 1, thr, -1, half) == 1             # ns outside 0 .. 8
        assert call(tp, -1, 1, thr, 9, half) == 1
        assert call(tp, -1, 1, thr, 1, None) == 1
        for hw in bad_half:                                    # a half-width outside 0 .. 32
            assert call(tp, -1, 1, thr, 2, hw) == 1
        assert call(tp, -1, 16, thr, 8, half) == 0             # the largest call is fine
    assert begin(tp, -1, 1, thr, 0, None, 2) == 1              # fields must be 0 or 1
    assert lib.csim_ensemble_verify_spatial_wait(e._h, None, None, None, None, None, None) == 0  # the good _begin above
    assert lib.csim_ensemble_verify_spatial_wait(e._h, None, None, None, None, None, None) == 4  # nothing in flight
    with pytest.raises(ValueError):
        e.verify_spatial(np.zeros((3, 3)), thresholds=[0.5])
    e.close()

    one = ensemble_with(csim, random_fields(1, 4, 4, seed=82))  # its only member as the truth leaves no forecast
    assert lib.csim_ensemble_verify_spatial(one._h, None, 0, 1, thr, 0, None, None, None, None, None, None, None) == 1
    one.close()


def test_member_and_overflow_limits(csim):
    lib, C = csim.lib(), csim.C
    thr = (C.c_double * 1)(0.5)
    big = csim.Ensemble(4098, 1, 1)              # zero-filled members
    truth = np.zeros((3, 3))
    tp = truth.ctypes.data_as(C.POINTER(C.c_double))
    none = [None] * 6
    assert lib.csim_ensemble_verify_spatial(big._h, tp, -1, 1, thr, 0, None, *none) == 5        # M = 4098
    assert lib.csim_ensemble_verify_spatial(big._h, None, 7, 1, thr, 0, None, *none) == 5       # M = 4097
    assert lib.csim_ensemble_verify_spatial_begin(big._h, None, 7, 1, thr, 0, None, 0) == 5
    assert lib.csim_ensemble_verify_spatial_wait(big._h, *none) == 4
    big.close()
    # 4096 members on 125 x 125: half = 32 is past the bound, half = 31 inside it (and takes the score pass's largest
    # histogram and a table of 95 x 95 into LDS)
    nx = ny = 125
    assert not csim.verify_spatial_limit(4096, nx, ny, 32) and csim.verify_spatial_limit(4096, nx, ny, 31)
    e = csim.Ensemble(4096, nx, ny)
    truth = np.zeros((ny + 2, nx + 2))
    truth[1:-1, 1:-1] = 1.0
    with pytest.raises(csim.CsimError) as err:
        e.verify_spatial(truth, thresholds=[0.5], half_widths=(0, 32))
    assert err.value.code == 5
    got = e.verify_spatial(truth, thresholds=[0.5, -0.5], half_widths=(31, 0))
    assert got.cells == nx * ny and got.nan_cells == 0
    assert got.table[0, 0, 1] == nx * ny and got.table[0].sum() == nx * ny      # nobody exceeds 0.5, the truth does
    assert got.table[1, 4096, 1] == nx * ny and got.table[1].sum() == nx * ny   # everybody exceeds -0.5
    want = ref.tables(np.full((1, ny, nx), 4096, dtype=np.int64), np.ones((1, ny, nx), dtype=np.int64),
                      np.zeros((ny, nx), dtype=bool), 4096, [31, 0])
    assert np.array_equal(got.nbh[1], want[1][0]) and not got.nbh[0, :, 0].any() and not got.nbh[0, :, 2].any()
    assert np.all(got.scores.fss[1] == 1.0) and np.all(got.scores.fss[0] == 0.0)
    e.close()
