"""What the order-statistic seam test (tests/test_gpu_order_stat_seams.py) reaches, checked on the CPU: the member
counts of tests/order_stat_cases.py against its restatement of for_sort_form, sort_tile and CSIM_LOAD_TILE
(csrc/ensemble_cell.hpp), its 0/1 and structured inputs, the levels that read every sorted position against the
library's own plan, and its grid shapes."""
import numpy as np
import pytest

import order_stat_cases as osc
from __graft_entry__ import load_package


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


def test_restated_forms_and_tiles():
    assert [osc.sort_form(n) for n in (1, 2, 3, 4, 5, 64, 65, 128, 129, 512, 513, 4096)] == [
        ("lane", 1), ("lane", 2), ("lane", 4), ("lane", 4), ("lane", 8), ("lane", 64), ("wave", 2), ("wave", 2),
        ("wave", 4), ("wave", 8), ("wave", 16), ("wave", 64)]
    assert osc.sort_tile(100) == (16, 101, 16 * 101 * 8)
    assert osc.sort_tile(511) == (16, 511, 65408) and osc.sort_tile(512) == (8, 513, 32832)
    assert osc.sort_tile(4096) == (4, 4097, 131104)
    # the largest verification: a truth member and 4096 others, the histogram's 4097 bins behind the tile
    assert osc.tile_of("verify_member", 4097) == (4, 4097, 4 * 4097 * 8 + 4 * 4097)
    assert osc.tile_of("verify_truth", 495)[2] == 65344 and osc.tile_of("verify_truth", 496)[0] == 8


def test_every_network_is_filled():
    """every lane P and every wave E at its smallest count, full, and one past it, for the quantiles (B values), the
    verification against a host truth (B) and against a truth member (B - 1)"""
    S = set(osc.MEMBER_SEAMS)
    assert osc.MEMBER_SEAMS == sorted(S) and 55 <= len(S) <= 80, len(S)
    for kind in osc.KINDS:
        sorted_counts = {osc.forecast(kind, B) for B in S if osc.forecast(kind, B) >= 1}
        for P in osc.LANE_P:
            assert P in sorted_counts and osc.sort_form(P) == ("lane", P), (kind, P)
        for E in osc.WAVE_E:
            if (kind, E) != ("verify_member", 64):   # B = 4097, which the quantiles refuse: TRUTH_LANE_MEMBERS has it
                assert 64 * E in sorted_counts and osc.sort_form(64 * E) == ("wave", E), (kind, E)
    assert osc.TRUTH_LANE_MEMBERS == [513, 1025, 4097]
    for P in osc.LANE_P[1:]:
        assert P // 2 + 1 in S and osc.sort_form(P // 2 + 1) == ("lane", P)
    for E in osc.WAVE_E:
        assert 32 * E + 1 in S and osc.sort_form(32 * E + 1) == ("wave", E)
    assert [B for B in osc.MEMBER_SEAMS if B > 1025] == [1026, 1984, 1985, 2047, 2048, 2049, 3072, 4095, 4096]


def test_both_sides_of_every_tile_switch():
    want = {"quantiles": [(511, 512), (1023, 1024)], "verify_truth": [(495, 496), (963, 964)],
            "verify_member": [(495, 496), (963, 964)]}   # (with a truth member: M = 494 / 495 and 962 / 963)
    S = set(osc.MEMBER_SEAMS)
    for kind in osc.KINDS:
        sw = osc.ct_switches(kind)
        assert sw == want[kind], kind
        assert [osc.tile_of(kind, lo)[0] for lo, _ in sw] == [16, 8] and osc.tile_of(kind, sw[-1][1])[0] == 4
        for lo, hi in sw:
            assert set(range(lo - 2, hi + 3)) <= S
            ct, _, lds = osc.tile_of(kind, lo)
            ct_hi, stride_hi, lds_hi = osc.tile_of(kind, hi)
            assert lds <= osc.SORT_LDS_BUDGET < lds_hi + (ct - ct_hi) * stride_hi * 8   # hi with lo's ct: too large
    # a tile never exceeds the 160 KiB of a workgroup
    largest = [osc.tile_of("quantiles", 4096), osc.tile_of("verify_truth", 4096), osc.tile_of("verify_member", 4097)]
    assert max(t[2] for t in largest) == 147492 <= 160 * 1024


def test_loader_trip_edges():
    """CSIM_LOAD_TILE's eight-deep loop: the listed counts straddle the first thread's first and second trip and the
    count at which every thread has made its first, for each step the loader takes"""
    S = set(osc.MEMBER_SEAMS)
    assert osc.loader_changes(16)[:3] == [113, 128, 241]
    assert osc.loader_changes(32)[:3] == [737, 768, 993]
    assert osc.loader_changes(64)[-2:] == [1985, 2048]
    assert {112, 113, 127, 128, 129, 240, 241, 736, 737, 767, 768, 769, 992, 993, 1984, 1985, 2047, 2048, 2049} <= S
    # the restated trips against a plain replay of the macro's loops: every member loaded exactly once
    for members, ct in ((112, 16), (113, 16), (128, 16), (129, 16), (241, 16), (737, 8), (768, 8), (1985, 4)):
        step, seen = 256 // ct, np.zeros(members, dtype=int)
        for m0 in range(step):
            m, trips = m0, 0
            while m + 7 * step < members:
                seen[[m + u * step for u in range(8)]] += 1
                m += 8 * step
                trips += 1
            assert trips == osc.loader_trips(members, step, m0), (members, m0)
            while m < members:
                seen[m] += 1
                m += step
        assert (seen == 1).all(), members


def test_exhaustive_patterns_are_all_there():
    for M in range(1, 17):
        a = osc.zero_one_exhaustive(M)
        assert a.shape[0] == M and a.shape[1] >= 3 and a.shape[2] >= 3 and set(np.unique(a)) <= {0.0, 1.0}
        cols = a.reshape(M, -1)
        codes = (cols.astype(np.int64) * (1 << np.arange(M))[:, None]).sum(axis=0)
        assert np.array_equal(codes[: 1 << M], np.arange(1 << M)), M
        assert cols.shape[1] < max(10, 2 << M)
    assert osc.zero_one_exhaustive(16).shape == (16, 256, 256)   # a 254 x 254 grid


def test_counted_patterns():
    for M in (1, 2, 65, 512, 1024):
        cols = osc.zero_one_counts(M, 2)
        assert cols.shape == (M, 2 * (M + 1)) and set(np.unique(cols)) <= {0.0, 1.0}
        assert np.array_equal(cols.sum(axis=0), np.repeat(np.arange(M + 1), 2))
    cols = osc.zero_one_counts(512, 2)
    assert not np.array_equal(cols[:, 200], cols[:, 201])       # two placements of one count
    assert not np.array_equal(cols[:, 200], np.sort(cols[:, 200]))
    for M in (1025, 2048, 4096):
        js = osc.zero_one_count_list(M)
        last = (M - 1) // 64 * 64
        assert {0, 1, M - 1, M, 63, 64, 65, last - 1, last, last + 1} <= set(js) and len(js) <= 3 * M // 64 + 4
        assert np.array_equal(osc.zero_one_counts(M, 1).sum(axis=0), js)
    assert np.array_equal(osc.zero_one_counts(300, 1, seed=5), osc.zero_one_counts(300, 1, seed=5))
    assert not np.array_equal(osc.zero_one_counts(300, 1, seed=5), osc.zero_one_counts(300, 1, seed=6))


@pytest.mark.parametrize("M", [1, 2, 3, 64, 65, 300, 1024])
def test_structured_patterns(M):
    cols, names, n_distinct = osc.structured(M)
    assert cols.shape == (M, len(names)) and len(set(names)) == len(names)
    asc = cols[:, 0]
    for k in range(n_distinct):   # permutations of one set of distinct finite values
        assert np.isfinite(cols[:, k]).all() and np.array_equal(np.sort(cols[:, k]), asc), names[k]
    assert len(np.unique(asc)) == M
    assert np.array_equal(cols[:, 1], asc[::-1])
    rot = [n for n in names if n.startswith("rotated")]
    assert len(rot) == len({s for r in range(64, M, 64) for s in (r - 1, r, r + 1) if 0 < s < M})
    if M >= 300:
        assert np.array_equal(cols[:, names.index("rotated by 65")], np.roll(asc, 65))
        organ = cols[:, names.index("organ pipe")]
        assert organ.argmax() in (M // 2 - 1, M // 2, (M + 1) // 2) and organ[0] == asc[0]
    ties = {n: cols[:, names.index(n)] for n in names[n_distinct:]}
    assert np.isinf(ties["a third +inf, first"]).sum() == max(1, M // 3)
    assert np.isinf(ties["all but one +inf"]).sum() == M - 1
    z = ties["signed zeros"]
    assert (z == 0).all() and (M < 64 or 0 < np.signbit(z).sum() < M)
    assert len(np.unique(ties["three values"])) <= 3 and len(np.unique(ties["all equal"])) == 1
    assert not np.isnan(cols).any()


def test_bit_reversed_order():
    assert list(osc.bit_reversed(8)) == [0, 4, 2, 6, 1, 5, 3, 7]
    assert sorted(osc.bit_reversed(300)) == list(range(300)) and list(osc.bit_reversed(300)[:3]) == [0, 256, 128]


def test_pack():
    cols = np.arange(3 * 100, dtype=np.float64).reshape(3, 100)
    a = osc.pack(cols)
    assert a.shape == (3, 3, osc.PACK_ROW)
    flat = a.reshape(3, -1)
    assert np.array_equal(flat[:, :100], cols) and np.array_equal(flat[:, 100:], cols[:, :11])
    assert osc.pack(np.zeros((2, 5))).shape == (2, 3, osc.PACK_ROW)
    assert osc.CELL_CAP * osc.SORT_MAX_VALUES * 8 < 150e6
    with pytest.raises(AssertionError):
        osc.pack(np.zeros((1, osc.CELL_CAP + 1)))


@pytest.mark.parametrize("M", osc.MEMBER_SEAMS)
def test_all_positions_are_read(csim, M):
    """the plan of the levels k / (M - 1) names every index k as `lo` with g < 0.5 or as `hi` with g >= 0.5, the end
    of numpy's interpolation that carries the value: equality with np.quantile then pins every sorted value"""
    calls = osc.all_positions_levels(M)
    assert all(1 <= len(c) <= osc.MAX_LEVELS for c in calls) and sum(map(len, calls)) == M
    named = set()
    for qs in calls:
        lo, hi, g = csim.ensemble_quantile_plan(M, qs)
        named |= {l if gg < 0.5 else h for l, h, gg in zip(lo, hi, g)}
    assert named == set(range(M))


@pytest.mark.parametrize("M", osc.MEMBER_SEAMS)
def test_sorted_quantiles_is_np_quantile(M):
    """the GPU test's reference for all positions of a count, one np.sort, against np.quantile level by level, bit for
    bit: distinct values, ties, infinities of both signs, zeros of both signs, a NaN member"""
    rng = np.random.default_rng(M)
    a = rng.standard_normal((M, 2, 5))
    a[:, 0, 1] = rng.choice([-1.0, 0.0, -0.0, 1.0], M)
    a[: max(1, M // 3), 0, 2] = np.inf
    a[M // 2:, 0, 3] = -np.inf
    a[M // 2, 0, 4] = np.nan
    a[:, 1, 0] = rng.integers(0, 2, M)
    a[:, 1, 1] = np.inf
    qs = np.concatenate(osc.all_positions_levels(M))
    if M > 300:   # np.quantile level by level costs a partition each: a spread of positions, both ends among them
        qs = np.concatenate([qs[:40], qs[rng.integers(0, M, 80)], qs[-40:]])
    got = osc.sorted_quantiles(a, qs)
    with np.errstate(all="ignore"):
        want = np.array([np.quantile(a, q, axis=0) for q in qs])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want[:, 0, 4]).all()
    ok = ~np.isnan(want) & (want != 0)   # (the sign of a zero quantile is whatever numpy's partition left)
    assert np.array_equal(got[ok].view(np.int64), want[ok].view(np.int64))
    assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


def test_layout_shapes():
    shapes = osc.LAYOUT_SHAPES
    assert len(shapes) == 20 and len(set(shapes)) == 20
    for nx2 in (63, 64, 65, 127, 128, 129):
        cells = sorted((nx + 2) * (ny + 2) for nx, ny in shapes if nx + 2 == nx2)
        assert len(cells) == 3 and cells[1] % 256 == 0 and cells[0] == cells[1] - nx2 and cells[2] == cells[1] + nx2
    assert all(nx >= 1 and ny >= 1 for nx, ny in shapes)
    assert (1, 300) in shapes and 64 // 3 == 21 and (1000, 1) in shapes
    (a, b), (c, d) = osc.GRID_MAX_SHAPES
    assert (a + 2) * (b + 2) == osc.VERIFY_GRID_MAX * osc.VERIFY_LANE_CELLS
    assert -(-(c + 2) * (d + 2) // osc.VERIFY_LANE_CELLS) == osc.VERIFY_GRID_MAX + 1
