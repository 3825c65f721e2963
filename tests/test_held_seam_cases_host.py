"""tests/held_seam_cases.py held to its word without a GPU: what every case of the table says it reaches (blocks, rows
of the last block, 64 % M, 256 % M, M % 4, the carry branches of the two staging walks) against an emulation from the
constants; the table as a whole; the recipes against those of tests/test_gpu_held.py; the inputs (several plan levels,
distinct values, the inactive tenth, a plan order that moves observations across 64-row blocks, rejections outside the
first block); and that the reference tells five wrong kernels from the right one, bit for bit, with every excuse shown
to be one."""
import numpy as np
import pytest

import held_seam_cases as hc
import screen_restatement as screen
from __graft_entry__ import load_package

IDS = [hc.name(c) for c in hc.CASES]


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


def exact_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("c", hc.CASES, ids=IDS)
def test_a_case_reaches_what_the_table_says(c):
    got = hc.reaches(c.M, c.nobs)
    print(hc.name(c), "blocks, last, 64 % M, 256 % M, M % 4, carry of 64 lanes, carry of 256 lanes:", got)
    assert got == (c.blocks, c.last_rows, c.r64, c.r256, c.r4, c.carry64, c.carry256)
    assert 2 <= c.M <= hc.MAX_MEMBERS and hc.held_lds_bytes(c.M) <= 160 * 1024
    assert c.path in ("host", "both") and c.truth in (None, "first", "middle", "last")


def test_the_table_as_a_whole():
    pairs = [(c.M, c.nobs) for c in hc.CASES]
    assert pairs == [(6, 1), (2, 129), (3, 65), (7, 63), (7, 64), (63, 65), (64, 128), (65, 129), (129, 65), (255, 65),
                     (256, 129)]
    assert {c.r4 for c in hc.CASES} == {0, 1, 2, 3}
    assert any(c.M <= 64 and c.blocks > 1 for c in hc.CASES) and any(c.M > 64 and c.blocks > 1 for c in hc.CASES)
    # the tail clamps rr[u] twice at M % 4 = 3, also below HELD_RB; full blocks, a second block, a tail of one row
    assert any(c.r4 == 3 and c.M < hc.HELD_RB for c in hc.CASES) and any(c.r4 == 3 and c.M > 64 for c in hc.CASES)
    assert any(c.last_rows == hc.HELD_ROWS and c.blocks == 1 for c in hc.CASES)
    assert any(c.last_rows == hc.HELD_ROWS and c.blocks == 2 for c in hc.CASES)
    assert any(c.last_rows == 1 and c.blocks == 3 for c in hc.CASES)
    # both carries taken and not taken, on either side of a wave of members
    for field in ("carry64", "carry256"):
        assert {getattr(c, field) for c in hc.CASES} == {False, True}
    assert any(c.carry64 and c.M < 64 for c in hc.CASES) and any(c.carry64 and c.M > 64 for c in hc.CASES)
    # the largest request is the limit's
    assert hc.held_lds_bytes(max(c.M for c in hc.CASES)) == hc.held_lds_bytes(hc.MAX_MEMBERS) == 133120
    # paths, truth members and kinds
    for pair in hc.DEVICE_REQUIRED + [(6, 1)]:
        assert hc.case_of(*pair).path == "both"
    assert {c.truth for c in hc.CASES} == {None, "first", "middle", "last"}
    assert sorted(c.kind for c in hc.CASES if c.kind != "point") == ["bilinear", "box"]
    assert all(c.kind == "point" for c in hc.CASES if c.M > 7)


def test_the_recipes_are_those_of_test_gpu_held(csim):
    import test_gpu_held as tgh

    assert hc.GRID[4] == tgh.GRID[4] == 2.5
    assert exact_bits(hc.members(9, hc.GRID, 5), tgh.members(9, hc.GRID, 5))
    for kind in ("bilinear", "box"):
        a = hc.linear_network(csim, np.random.default_rng(3), hc.GRID, kind, 65)
        b = tgh.make_network(csim, np.random.default_rng(3), hc.GRID, kind, 65)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and exact_bits(a[3], b[3])
        assert len(a[2]) == len(b[2]) and all(np.array_equal(p, q) for p, q in zip(a[2], b[2]))


@pytest.mark.parametrize("c", hc.CASES, ids=IDS)
def test_the_inputs_of_a_case(csim, c):
    x = hc.inputs(csim, c)
    nobs, M = c.nobs, c.M
    assert x.H.shape == (nobs, M) and x.X0.shape == x.X1.shape == (x.B, 18, 18)
    assert x.B == M + (c.truth is not None) and (x.t is None) == (c.truth is None)
    # every value of the members, and so of a point network's rows, is distinct
    for X in (x.X0, x.X1):
        assert np.unique(X).size == X.size
    if c.kind == "point":
        assert np.unique(x.H).size == x.H.size
    else:   # two stations may share a cell there, as in tests/test_gpu_held.py; within a row every value is distinct
        assert all(np.unique(row).size == M for row in x.H)
    # the plan: several levels wherever two windows can overlap; its order is a permutation
    order, (lx, ly) = hc.plan_order(csim, x.i, x.j)
    lev = np.asarray(csim.ensemble_assim_plan(x.i, x.j, lx, ly))
    assert np.array_equal(order, x.order) and np.array_equal(np.sort(order), np.arange(nobs))
    assert np.array_equal(x.order[x.pos], np.arange(nobs))
    assert lx >= 1 and ly >= 1
    if nobs > 1:
        assert lev.max() >= 1
    if nobs > hc.HELD_ROWS:
        assert not np.array_equal(order, np.arange(nobs))
        moved = np.flatnonzero(hc.block_of(x.pos) != hc.block_of(np.arange(nobs)))
        print(hc.name(c), f"{lev.max() + 1} levels, {len(moved)} observations change their block")
        assert len(moved) >= 1
    # the inactive: about a tenth, never none, never a whole block
    inactive = np.count_nonzero(x.mask == 0)
    if nobs == 1:
        assert inactive == 0     # its only row is its only block
    else:
        assert 1 <= inactive <= max(2, nobs // 5)
    for blocks in (hc.block_of(x.pos), hc.block_of(np.arange(nobs))):
        for b in np.unique(blocks):
            assert x.mask[blocks == b].any()
    assert x.mask[x.order[-1]] == 1
    # the slots, and the rows from their states
    assert set(x.slot.tolist()) == ({0} if nobs == 1 else {0, 1})
    for o in (0, nobs - 1):
        S = (x.X0, x.X1)[x.slot[o]]
        assert exact_bits(x.H[o], hc.operator(S, x.t, x.i, x.j, x.taps)[:, o])
    # the gross errors are rejected, one of them outside the first block where there is another
    st = x.status
    assert np.array_equal(st == screen.INACTIVE, x.mask == 0)
    assert np.array_equal(np.flatnonzero(st == screen.REJECTED), np.sort(x.gross))
    if nobs > 1:
        assert len(x.gross) == 2 and np.count_nonzero(st == screen.USED) >= 2
    if c.blocks > 1:
        assert hc.block_of(x.pos[x.gross]).max() >= 1 and hc.block_of(x.pos[x.gross]).min() == 0
    # every block keeps a used row but a tail of one row that is rejected
    for b in range(c.blocks):
        rows = x.order[b * hc.HELD_ROWS:(b + 1) * hc.HELD_ROWS]
        assert (st[rows] == screen.USED).any() or (len(rows) == 1 and st[rows[0]] == screen.REJECTED)


@pytest.mark.parametrize("c,device", hc.RUNS, ids=hc.RUN_IDS)
def test_the_reference_tells_wrong_kernels_from_the_right_one(csim, c, device):
    x = hc.inputs(csim, c)
    W, wbar = hc.weights(csim, c, device)
    assert np.isfinite(W).all() and np.isfinite(wbar).all()
    right = hc.right_results(x, W, wbar)
    assert not exact_bits(right[0], x.H)           # the analysis moves the rows
    wrong = hc.wrong_variants(x, W, wbar)
    excused = hc.excused(c)
    assert set(wrong) == set(hc.VARIANTS) and set(excused) <= set(hc.VARIANTS) and len(excused) <= 2
    for v in hc.VARIANTS:
        if v in excused:
            assert not hc.differs(wrong[v], right), (v, excused[v])   # an excuse is one: the variant is the right result
        else:
            assert hc.differs(wrong[v], right), v
    # what each variant is aimed at
    for v in ("last_block_untransformed", "block_from_block_0", "tail_outputs_as_last", "row_rotated"):
        assert v in excused or not exact_bits(wrong[v][0], right[0]), v
    if "mv_at_plan_position" not in excused:
        assert not exact_bits(wrong["mv_at_plan_position"][1], right[1])
        assert not exact_bits(wrong["mv_at_plan_position"][2], right[2])


def test_the_gram_seams_sit_where_they_are_named(csim):
    import etkf_restatement as etkf

    assert {5, 89, 125, 177, 181} <= set(hc.GRAM_COLS)
    for cols in hc.GRAM_COLS:
        assert hc.gram_blocks(cols) == hc.GRAM_BLOCKS[cols]
    # one workgroup of 256 lanes -> two with one, two and four blocks a lane; the step of the side 1 -> 2 and 45 -> 46
    assert hc.gram_blocks(4) == 1 and hc.gram_blocks(5) == 3
    assert hc.gram_blocks(88) <= 256 < hc.gram_blocks(89)
    assert hc.gram_blocks(124) <= 512 < hc.gram_blocks(125)
    assert hc.gram_blocks(176) <= 1024 < hc.gram_blocks(177)
    assert hc.gram_blocks(180) == 1035 == hc.gram_blocks(177) and hc.gram_blocks(181) == 1081
    for cols in hc.GRAM_COLS:
        for nobs in hc.GRAM_NOBS:
            assert csim.obs_gram_plan(cols - 1, nobs) == etkf.gram_plan(cols - 1, nobs) == (-(-nobs // 64),) * 2
            g = hc.gram_inputs(csim, cols, nobs)
            assert not np.array_equal(g.order, np.arange(nobs)) and set(g.slot.tolist()) == {0, 1}
            assert 1 <= np.count_nonzero(g.mask == 0) < nobs // 5 and g.mask[g.order[-1]] == 1
            # the carry of the 256-lane staging walk is taken wherever 256 % M is not 0 and a segment is longer than a trip
            assert hc.walk_carries(g.M, hc.GRAM_THREADS, 64) == (256 % g.M != 0)
