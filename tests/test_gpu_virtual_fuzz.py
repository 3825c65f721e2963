"""Decomposed runs on process grids of 2 .. 16 virtual ranks against the oracle, bit for bit: every rank is a real
external-halo csim_stepper on its own tile in this process, faces routed host-side (tests/virtual_ranks.py).  The cases
are a seeded fuzz and a fixed list at the strip seams, the capped depths, 3 x 3 .. 4 x 4 grids, chains and the screened
bodies (tests/virtual_fuzz_cases.py; what they reach is checked on the CPU by tests/test_virtual_fuzz_cases_host.py).

The oracle is decomposition-invariant: every tile's interior and the ghost lines of its physical sides are a window of
run_single on the global field; its neighbour-side ghost lines are those of oracle World's tile.

Not covered here: the RCCL schedules (frame / bulk split, relay, merged launch) on such tiles — an external-halo pass
plans the whole tile as one launch, and RCCL refuses two ranks on one device."""
import os

import numpy as np
import pytest

from oracle import cpu_oracle as ora
from virtual_fuzz_cases import (DEFAULT_SEED, SEAMS, WORLDS, describe, fuse_limit, fuzz_cases, initial_interior,
                                tile_cap)
from virtual_ranks import VirtualRanks, physical_mask, tile_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def csim():
    from __graft_entry__ import load_package
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def differing(got, want, mask):
    """(number of cells under the mask whose bits differ — NaN by position —, the first of them as (row, column))"""
    nan = np.isnan(want)
    bad = mask & np.where(nan, ~np.isnan(got), got.view(np.int64) != want.view(np.int64))
    where = np.argwhere(bad)
    return len(where), (tuple(int(v) for v in where[0]) if len(where) else None)


def run_case(csim, c):
    world, nx, ny, steps, value = c["world"], c["nx"], c["ny"], c["steps"], c["value"]
    bc = csim.bc_codes(c["bc"])
    phys = (c["dx"], c["dy"], c["D"], c["vx"], c["vy"], c["dt"])
    u0 = initial_interior(c)
    single = np.zeros((ny + 2, nx + 2))
    single[1:-1, 1:-1] = u0
    ora.run_single(single, *phys, bc, steps, value)
    tiled = None
    if value == 0.0 and not np.signbit(value):   # the oracle's tiles take the reference driver's Dirichlet value
        tiled = ora.World(world, nx, ny, c["dx"], c["dy"])
        tiled.scatter(u0)
        tiled.run(c["D"], c["vx"], c["vy"], c["dt"], bc, steps)
    vr = VirtualRanks(csim, world, nx, ny, c["dx"], c["dy"], bc, value, fuse=c["fuse"], opts=c["opts"])
    try:
        assert vr.depth == fuse_limit(c), (describe(c), vr.depth)
        if "cap" in c:
            smallest = min(min(dec.nx_local, dec.ny_local) for dec in vr.decs)
            assert vr.depth == smallest == c["cap"] == min(tile_cap(c)), (describe(c), vr.depth, smallest)
        vr.upload_global(u0)
        for n in c["calls"]:
            vr.advance(c["D"], c["dt"], c["vx"], c["vy"], n)
        for r, dec in enumerate(vr.decs):
            got = vr.download(r)
            window = single[dec.y_offset:dec.y_offset + dec.ny_local + 2, dec.x_offset:dec.x_offset + dec.nx_local + 2]
            n, first = differing(got, window, physical_mask(dec))
            assert n == 0, (describe(c), "vs the global run", r, list(dec.coords), n, first)
            if tiled is not None:
                n, first = differing(got, tiled.tile(r), tile_mask(dec))
                assert n == 0, (describe(c), "vs the oracle's tile", r, list(dec.coords), n, first)
        assert vr.checksum() == csim.checksum_host(single[1:-1, 1:-1]), describe(c)
        if steps > 0:
            allowed = c["opts"]["pow2_v"] == 1 and c["opts"]["fused_2c"] == 1 and \
                csim.pow2_velocity_screen(c["D"], c["dt"], c["vx"], c["vy"], c["dx"], c["dy"])[0] > 0.0
            active = {st.get_option("pow2_v_active") for st in vr.st}
            assert active == {int(allowed)}, (describe(c), active)
    finally:
        vr.close()


@pytest.mark.parametrize("world", WORLDS)
def test_fuzz_tiles_equal_the_oracle(csim, world):
    seed = int(os.environ.get("CSIM_FUZZ_SEED", DEFAULT_SEED))   # (other seeds: extended soak runs)
    cases = [c for c in fuzz_cases(seed) if c["world"] == world]
    assert len(cases) >= 5
    for c in cases:
        run_case(csim, c)


@pytest.mark.parametrize("c", SEAMS, ids=[f"{c['case']}-np{c['world']}-{c['nx']}x{c['ny']}-T{c['fuse']}" for c in SEAMS])
def test_seam_tiles_equal_the_oracle(csim, c):
    run_case(csim, c)
