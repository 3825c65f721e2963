"""What the decomposed-run fuzz (tests/test_gpu_virtual_fuzz.py) reaches, checked on the CPU: its cases
(tests/virtual_fuzz_cases.py) are pure, so every rank's tile, its physical and neighbour sides and the passes that
VirtualRanks.advance would take can be classified without a GPU.  `python tests/test_virtual_fuzz_cases_host.py`
prints the coverage numbers."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from __graft_entry__ import load_package
from oracle import cpu_oracle as ora
from virtual_fuzz_cases import (DEFAULT_SEED, FUZZ_PER_WORLD, SEAMS, STRIDE, VALUES, WORLDS, div_mode, fuse_limit,
                                fuzz_cases, grid_dims, initial_interior, schedule, tile_cap, tiles)

SIDES = ("left", "right", "down", "up")
CORNERS = [(0, 2), (1, 2), (0, 3), (1, 3)]   # (x side, y side) of the corners BL, BR, TL, TR


def _sign(v):
    return (v > 0) - (v < 0)


def coverage(csim):
    cases = fuzz_cases(DEFAULT_SEED) + SEAMS
    r = dict(cases=len(cases), worlds={w: 0 for w in WORLDS}, side_keys=set(), corner_keys=set(), depths={}, caps=set(),
             depth1_only=0, four_nbr_wide=0, three_nbr=0, chain_end=0, chain_middle=0, stride_widths=set(),
             right_parity=set(), unequal=set(), signs=set(), minus_zero=set(), D0=0, dirichlet_values=set(), splits=0,
             steps=set(), p2_active=0, p2_refused=0)
    for c in cases:
        world, nx, ny = c["world"], c["nx"], c["ny"]
        px, py = grid_dims(world)
        mine = tiles(world, nx, ny)
        for rank, t in enumerate(mine):   # the restatement against the library and the oracle, rank by rank
            assert t == ora.decomp(world, rank, nx, ny) == csim.decomp_init(world, rank, nx, ny).as_dict(), (c, rank)
        assert sum(c["calls"]) == c["steps"] and nx * ny <= 600_000 and min(tile_cap(c)) >= 2
        passes = {t for call in schedule(c) for t in call}
        fused = {t for t in passes if t >= 2}
        mode = div_mode(c["dx"], c["dy"])
        r["worlds"][world] += 1
        for t in fused:
            r["depths"][(mode, t)] = r["depths"].get((mode, t), 0) + 1
        r["depth1_only"] += c["steps"] >= 3 and not fused
        bx, by = tile_cap(c)
        cap = min(bx, by)
        if cap < 7 and cap in fused and bx != by:
            r["caps"].add((cap, "x" if bx < by else "y"))
        r["unequal"] |= {"x"} if nx % px else set()
        r["unequal"] |= {"y"} if ny % py else set()
        r["signs"].add((_sign(c["vx"]), _sign(c["vy"])))
        r["minus_zero"] |= {k for k in ("vx", "vy") if repr(c[k]) == "-0.0"}
        r["D0"] += c["D"] == 0.0
        if "d" in c["bc"]:   # every side of the domain is some rank's physical side
            r["dirichlet_values"].add(repr(c["value"]))
        r["splits"] += len(c["calls"]) > 1
        r["steps"].add(c["steps"])
        if fused and c["opts"]["pow2_v"] == 1:
            allowed = c["opts"]["fused_2c"] == 1 and \
                csim.pow2_velocity_screen(c["D"], c["dt"], c["vx"], c["vy"], c["dx"], c["dy"])[0] > 0.0
            r["p2_active" if allowed else "p2_refused"] += 1
        for t in mine:
            kinds = tuple("N" if t[s] >= 0 else c["bc"][k] for k, s in enumerate(SIDES))
            r["side_keys"].add(kinds)
            for corner, (sx, sy) in enumerate(CORNERS):
                for phys, nbr in ((sx, sy), (sy, sx)):
                    if kinds[phys] != "N" and kinds[nbr] == "N":
                        r["corner_keys"].add((corner, "x" if phys < 2 else "y", kinds[phys]))
            if not fused:
                continue
            neighbours = kinds.count("N")
            strips = max(-(-t["nx_local"] // STRIDE[T]) for T in fused)
            r["four_nbr_wide"] += neighbours == 4 and strips >= 3
            r["three_nbr"] += neighbours == 3
            if py == 1 and px >= 3:
                r["chain_end"] += neighbours == 1
                r["chain_middle"] += neighbours == 2
            r["stride_widths"] |= {(T, t["nx_local"] - STRIDE[T]) for T in fused if abs(t["nx_local"] - STRIDE[T]) <= 1}
            if t["right"] < 0:
                r["right_parity"].add(t["nx_local"] & 1)
    return r


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


@pytest.fixture(scope="module")
def reached(csim):
    return coverage(csim)


def test_generator_is_a_pure_function_of_the_seed():
    a, b = fuzz_cases(DEFAULT_SEED, 3), fuzz_cases(DEFAULT_SEED, 3)
    assert repr(a) == repr(b) and len(a) == 3 * len(WORLDS)
    assert repr(fuzz_cases(DEFAULT_SEED + 1, 3)) != repr(a)
    assert repr(fuzz_cases(DEFAULT_SEED, FUZZ_PER_WORLD)[:len(a)]) == repr(a)   # a shorter run is a prefix
    for c in a:
        assert (initial_interior(c) == initial_interior(c)).all() and initial_interior(c).shape == (c["ny"], c["nx"])


def test_the_schedule_restatement_on_known_runs():
    """VirtualRanks.advance by hand: 20 steps at depth 7 are 7 + 7 + 5 and a single step, a pass never takes the last
    step, fewer than three steps are single steps, and a 5-cell tile caps the depth"""
    base = dict(world=4, nx=400, ny=60, calls=[20], fuse=7)
    assert schedule(base) == [[7, 7, 5, 1]]
    assert schedule(dict(base, calls=[8, 2, 3])) == [[7, 1], [1, 1], [2, 1]]
    assert schedule(dict(base, fuse=None)) == [[6, 6, 6, 1, 1]] and fuse_limit(dict(base, fuse=None)) == 6
    assert schedule(dict(base, fuse=0, calls=[4])) == [[1, 1, 1, 1]]
    assert fuse_limit(dict(base, nx=10)) == 5 and schedule(dict(base, nx=10, calls=[7])) == [[5, 1, 1]]


def test_every_world_size_and_process_grid(reached):
    assert all(n >= 5 for n in reached["worlds"].values()), reached["worlds"]
    assert [grid_dims(w) for w in (5, 7, 9, 12, 16)] == [(5, 1), (7, 1), (3, 3), (4, 3), (4, 4)]


def test_tiles_by_their_neighbour_sides(reached):
    assert reached["four_nbr_wide"] >= 5    # eight distinct peers, three or more strips
    assert reached["three_nbr"] >= 20
    assert reached["chain_end"] >= 10 and reached["chain_middle"] >= 10


def test_every_bc_kind_beside_a_neighbour_side_at_every_corner(reached):
    """a physical side of each kind meets a neighbour side at each of the four corners, as the x side and as the y one"""
    want = {(corner, axis, kind) for corner in range(4) for axis in "xy" for kind in "dnp"}
    assert reached["corner_keys"] == want, sorted(want - reached["corner_keys"])
    # the kinds of a tile's four sides (N: a neighbour): every combination that a grid of two or more rows has — in x
    # and in y both neighbours, or a neighbour and a physical side of any kind — and every middle tile of a chain
    one_axis = [("N", "N")] + [("N", k) for k in "dnp"] + [(k, "N") for k in "dnp"]
    want = {x + y for x in one_axis for y in one_axis} | {("N", "N", a, b) for a in "dnp" for b in "dnp"}
    assert reached["side_keys"] >= want, sorted(want - reached["side_keys"])


def test_every_depth_in_every_division_mode(reached):
    want = {(mode, T) for mode in (0, 1, 2) for T in range(2, 8)}
    assert set(reached["depths"]) == want, sorted(want - set(reached["depths"]))
    assert reached["depth1_only"] >= 5


def test_caps_by_either_axis_with_a_pass_of_exactly_the_cap(reached):
    want = {(cap, axis) for cap in (2, 3, 4, 5, 6) for axis in "xy"}
    assert reached["caps"] >= want, sorted(want - reached["caps"])
    for c in SEAMS:
        if "cap" in c:
            assert c["cap"] == min(tile_cap(c)) == fuse_limit(c) < 7 and c["cap"] in schedule(c)[0]


def test_strip_seams_parities_and_unequal_tiles(reached):
    want = {(T, d) for T in (4, 6, 7) for d in (-1, 0, 1)}
    assert reached["stride_widths"] >= want, sorted(want - reached["stride_widths"])
    assert reached["right_parity"] == {0, 1}
    assert reached["unequal"] == {"x", "y"}


def test_sign_classes_values_and_run_lengths(reached):
    assert reached["signs"] == {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)}
    assert reached["minus_zero"] == {"vx", "vy"} and reached["D0"] >= 10
    assert reached["dirichlet_values"] == {repr(v) for v in VALUES}
    assert reached["splits"] >= 20 and reached["steps"] >= {0, 1, 2}


def test_screened_cases_take_the_fast_bodies_and_refuse_them(reached):
    """option pow2_v = 1 under a fused pass: with parameters that allow the 12-operation body and with ones that do not"""
    assert reached["p2_active"] >= 5 and reached["p2_refused"] >= 5
    screened = [c for c in SEAMS if c.get("field") == "screened"]
    assert {(c["world"], c["vx"], c["vy"]) for c in screened} == {
        (w, vx, vy) for w in (3, 9) for vx, vy in ((0.5, 0.25), (-0.5, -0.25), (0.5, 0.0), (0.0, 0.0))}
    assert {(c["opts"]["pow2_v"], c["opts"]["fused_2c"]) for c in screened} == {(1, 1), (0, 1), (1, 0)}
    for c in screened:
        u = initial_interior(c)
        t = tiles(c["world"], c["nx"], c["ny"])[c["world"] // 2]
        assert t["nx_local"] >= 3 * STRIDE[c["fuse"]] and sum(t[s] >= 0 for s in SIDES) == (2 if c["world"] == 3 else 4)
        mid = u[t["y_offset"]:t["y_offset"] + t["ny_local"], t["x_offset"]:t["x_offset"] + t["nx_local"]]
        assert (mid > 0).sum() > 0.95 * mid.size and ((mid == 0) & np.signbit(mid)).sum() == 120
        assert ((mid > 0) & (mid < 1e-249)).sum() == 120 and u.min() == 0.0


if __name__ == "__main__":
    pkg = load_package()
    pkg.build()
    got = coverage(pkg)
    for key, v in got.items():
        if key == "side_keys":
            v = len(v)
        elif key == "depths":
            v = {f"mode{m} T{t}": n for (m, t), n in sorted(v.items())}
        print(key, sorted(v) if isinstance(v, set) else v)
