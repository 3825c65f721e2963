"""Host side of the reduction tests (tests/test_gpu_reductions.py), no GPU needed: the numpy restatement of the sum's
order (tests/reduce_restatement.py) meets the derived bound against math.fsum at every shape the GPU tests use, it
really adds cells, rows and blocks (leaving one out changes its bits: sampled — the planted positions, the rows and
blocks at the ends and at the trips' seams, and a few random ones of each), and every planted position lies inside the
array it is planted in."""
import math

import numpy as np
import pytest

import reduce_restatement as rr

FIELD_CASES = [(nx, ny, rr.CAP_FIELD) for nx, ny in rr.SHAPES]
ENS_CASES = [(nx, ny, rr.CAP_ENSEMBLE) for nx, ny in rr.ENS_SHAPES]
ALL_CASES = FIELD_CASES + ENS_CASES
IDS = [f"{nx}x{ny}-cap{cap}" for nx, ny, cap in ALL_CASES]


def bits(x):
    return np.float64(x).view(np.int64)


@pytest.mark.parametrize("nx,ny,cap", ALL_CASES, ids=IDS)
def test_restated_sum_meets_the_derived_bound(nx, ny, cap):
    u = rr.field(nx, ny)
    got, want, bound = rr.restated_sum(u, cap), rr.ref_sum(u), rr.sum_bound(u, cap)
    assert math.isfinite(got) and abs(got - want) <= bound
    # the ghosts are not in it: the same interior in a ring of zeros gives the same bits
    v = np.zeros_like(u)
    v[1:-1, 1:-1] = u[1:-1, 1:-1]
    assert bits(rr.restated_sum(v, cap)) == bits(got)


def test_bound_counts_the_additions_of_the_longest_chain():
    # 130 x 1025: one column trip, two row trips, 6 butterfly steps, 3 wave adds, 1023 host adds
    assert rr.sum_additions(130, 1025, rr.CAP_FIELD) == 1 * 2 + 6 + 3 + 1023
    # 257 x 129 in the ensemble: two column trips, three row trips, 63 host adds
    assert rr.sum_additions(257, 129, rr.CAP_ENSEMBLE) == 2 * 3 + 6 + 3 + 63
    assert rr.sum_additions(1, 1, rr.CAP_FIELD) == 1 + 6 + 3
    assert [rr.trips(r, 1024) for r in (1, 1024, 1025, 2048, 2049)] == [1, 1, 2, 2, 3]


def test_restatement_is_exact_where_every_order_is():
    # integers: every partial sum is exact, so the order cannot matter
    rng = np.random.default_rng(5)
    u = rng.integers(-1000, 1000, size=(2051 + 2, 67 + 2)).astype(np.float64)
    assert rr.restated_sum(u) == float(u[1:-1, 1:-1].sum()) == rr.ref_sum(u)
    assert rr.restated_sum(u[:131, :], rr.CAP_ENSEMBLE) == float(u[1:130, 1:-1].sum())


def test_restatement_follows_the_stated_order():
    """2^53 and ones: 2^53 + 1 rounds back to 2^53, so the result tells in which order the values met"""
    big = 2.0 ** 53
    # two cells of one lane (columns 1 and 257 of one row): serial, big first -> the 1 is lost
    u = np.zeros((3, 300 + 2))
    u[1, 1], u[1, 257] = big, 1.0
    assert rr.restated_sum(u) == big
    # columns 1 and 2 hold big and -big, column 3 a 1: lanes 0 and 1 meet at mask 1, last, after lane 2 met lane 3
    u = np.zeros((3, 300 + 2))
    u[1, 1], u[1, 2], u[1, 3] = big, -big, 1.0
    # mask 2 first: lane 0 gets big + 1 = big (lost), lane 1 gets -big + 0; mask 1: big + -big = 0
    assert rr.restated_sum(u) == 0.0
    # three rows big, 1, -big: three blocks, added in order on the host -> (big + 1) + -big = 0 ...
    u = np.zeros((5, 3))
    u[1, 1], u[2, 1], u[3, 1] = big, 1.0, -big
    assert rr.restated_sum(u) == 0.0
    # ... but with a cap of two blocks, block 0 takes rows 0 and 2 (big + -big = 0) and block 1 keeps the 1
    assert rr.restated_sum(u, cap=2) == 1.0


def sample(n, k, rng, always=()):
    s = set(int(v) for v in always if 0 <= v < n)
    s.update(int(v) for v in rng.integers(0, n, size=k))
    return sorted(s)


@pytest.mark.parametrize("nx,ny,cap", ALL_CASES, ids=IDS)
def test_dropping_a_cell_a_row_or_a_block_changes_the_bits(nx, ny, cap):
    """sampled, not exhaustive: the planted cells and 4 random ones, the first and last rows, the rows at the trips'
    seams and 4 random ones, blocks 0, 1, G - 1 and 6 random ones"""
    u = rr.field(nx, ny)
    x = u[1:-1, 1:-1]
    G = min(ny, cap)
    parts = rr.block_partials(x, cap)
    whole = bits(rr.merge(parts))
    rng = np.random.default_rng([nx, ny, cap])
    cells = [(j - 1, i - 1) for j, i in list(rr.positions(nx, ny, cap).values()) + list(rr.lane_seats(nx, ny).values())
             if rr.is_interior((j, i), nx, ny)]
    cells += [(int(rng.integers(0, ny)), int(rng.integers(0, nx))) for _ in range(4)]
    for r, c in cells:
        keep = np.ones(x.shape, dtype=bool)
        keep[r, c] = False
        assert bits(rr.merge(rr.block_partials(x, cap, keep))) != whole, f"cell ({r}, {c})"
    for r in sample(ny, 4, rng, always=(0, ny - 1, G - 1, G, 2 * G)):
        keep = np.ones(x.shape, dtype=bool)
        keep[r, :] = False
        assert bits(rr.merge(rr.block_partials(x, cap, keep))) != whole, f"row {r}"
    if G > 1:
        for b in sample(G, 6, rng, always=(0, 1, G - 1)):
            assert bits(rr.merge(parts, skip=b)) != whole, f"block {b}"


@pytest.mark.parametrize("nx,ny,cap", ALL_CASES, ids=IDS)
def test_planted_positions_are_inside_the_array(nx, ny, cap):
    pos = rr.positions(nx, ny, cap)
    for label, (j, i) in list(pos.items()) + list(rr.lane_seats(nx, ny).items()):
        assert 0 <= j <= ny + 1 and 0 <= i <= nx + 1, label
    for label, p in rr.lane_seats(nx, ny).items():
        assert rr.is_interior(p, nx, ny), label
    # the corners and the ghost lines are ghosts, the trips' first rows exist exactly where the loop makes further trips
    for label in ("corner_bl", "corner_br", "corner_tl", "corner_tr", "ghost_bottom", "ghost_top", "ghost_left",
                  "ghost_right"):
        assert not rr.is_interior(pos[label], nx, ny)
    assert sum(k.startswith("whole_trip") for k in pos) == rr.trips(ny + 2, cap) - 1
    assert sum(k.startswith("interior_trip") for k in pos) == rr.trips(ny, cap) - 1
    for k, p in pos.items():
        if k.startswith("interior_trip") or k.startswith("col") or k in ("first", "last_row"):
            assert rr.is_interior(p, nx, ny), k


def test_the_shapes_make_the_trips_the_tests_are_about():
    t = {s: (rr.trips(s[1] + 2, rr.CAP_FIELD), rr.trips(s[1], rr.CAP_FIELD)) for s in rr.SHAPES}
    assert t[(130, 1022)] == (1, 1) and t[(130, 1023)] == (2, 1) and t[(130, 1024)] == (2, 1)
    assert t[(130, 1025)] == (2, 2) and t[(67, 2051)] == (3, 3) and t[(513, 62)] == (1, 1)
    e = {s: (rr.trips(s[1] + 2, rr.CAP_ENSEMBLE), rr.trips(s[1], rr.CAP_ENSEMBLE)) for s in rr.ENS_SHAPES}
    assert e[(1, 62)] == (1, 1) and e[(1, 63)] == (2, 1) and e[(257, 65)] == (2, 2) and e[(257, 129)] == (3, 3)


def test_references_on_non_finite_data():
    u = rr.field(5, 4)
    v = u.copy()
    assert rr.ref_linf(u, v) == 0.0
    v[2, 3] = np.nan
    assert math.isnan(rr.ref_linf(u, v)) and math.isnan(rr.ref_sum(v)) and math.isnan(rr.restated_sum(v))
    v[2, 3] = np.inf
    assert rr.ref_linf(u, v) == math.inf and rr.ref_sum(v) == math.inf and rr.restated_sum(v) == math.inf
    w = v.copy()
    assert math.isnan(rr.ref_linf(v, w))  # inf - inf
    # the reference's min / max skip NaN unless it is element 0
    v[2, 3] = np.nan
    assert rr.ref_minmax(v) == (u[np.isfinite(v)].min(), u[np.isfinite(v)].max())
    v[0, 0] = np.nan
    assert all(math.isnan(x) for x in rr.ref_minmax(v))
