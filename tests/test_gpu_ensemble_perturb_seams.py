"""csim_ensemble_perturb at its launch seams and in the far tail of its deviate, on the GPU, every comparison bit for
bit by integer view.

a. every targeted case and every fuzz case of tests/perturb_launch_cases.py (what they reach is checked on the CPU by
   tests/test_ensemble_perturb_launch_host.py) against the numpy restatement tests/perturb_restatement.py: all four
   instantiations of the kernel above 64 KiB of dynamic LDS, both 32-row ones at the largest launch (147 456 B), both
   sides of the automatic choice of the tile height, thin last tiles, periodic wraps, anisotropic radii, member shares;
b. the result does not depend on the tile height or on the member shares (options perturb_tile_rows,
   perturb_member_shares), and the options' own errors;
c. the current ping-pong buffer is the one perturbed, and two calls chain;
d. the r > 5 branch of the normal quantile on the device, at two cells found by a seed search on the CPU.

Measured on an MI355X: the whole file, 109 tests, takes 3.9 s of wall time (1.4 s of it loading the library), most of
the rest the numpy restatement."""
import numpy as np
import pytest

import perturb_launch_cases as plc
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


def where_differs(got, want):
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    return f"{len(bad)} values differ, the first at (member, row, column) {bad[0].tolist() if len(bad) else None}"


def perturbed(csim, c, X, tile_rows=None, shares=None):
    """the members after one perturb of case c on the state X, under the case's options or the given ones"""
    e = csim.Ensemble(c["B"], c["nx"], c["ny"], c["dx"], c["dy"], plc.bc_codes(c["bc"]), 0.25)
    try:
        e.upload_all(X)
        e.set_option("perturb_tile_rows", c["tile_rows"] if tile_rows is None else tile_rows)
        e.set_option("perturb_member_shares", c["shares"] if shares is None else shares)
        e.perturb(c["sigma"], c["corr_len"], c["seed"], c["draw"], centered=bool(c["centered"]), truth_member=c["t"])
        return e.download_all()
    finally:
        e.close()


def restated(c, X):
    return ref.perturb(X, c["seed"], c["draw"], c["sigma"], c["corr_len"], c["centered"], c["t"], c["dx"], c["dy"],
                       plc.bc_codes(c["bc"]))


# ---- a. the restatement ------------------------------------------------------------------------------------------

ALL_CASES = plc.SEAM_CASES + plc.fuzz_cases(plc.DEFAULT_SEED)


@pytest.mark.parametrize("case", ALL_CASES, ids=[c["name"] for c in ALL_CASES])
def test_restatement_bit_for_bit(csim, case):
    X = plc.start_state(case)
    got = perturbed(csim, case, X)
    want = restated(case, X)
    assert same_bits(got, want), where_differs(got, want)
    # ghost ring and the truth member: the uploaded bits, the negative zero of the interior included
    ring = np.ones(X.shape[1:], dtype=bool)
    ring[1:-1, 1:-1] = False
    assert same_bits(got[:, ring], X[:, ring])
    if case["t"] is not None:
        assert same_bits(got[case["t"]], X[case["t"]]) and np.signbit(got[case["t"], 1, 1])
    assert not same_bits(got, X)


# ---- b. the launch geometry is not in the result -----------------------------------------------------------------------

GEOMETRY_SETS = [
    plc.make(9, None, 130, 67, "nnnn", 1.0, 1.0, 16.2, 0, 2.0, 8, 1, name="R32_bounded"),
    plc.make(10, 3, 131, 45, "pppp", 1.0, 1.0, 2.0, 1, 0.25, (1 << 40) + 3, 7, name="R3_periodic_centered"),
    plc.make(9, 0, 70, 33, "dnpd", 1.0, 1.0, 0.0, 1, -0.5, 5, 2, name="R0_centered"),
    plc.make(12, None, 165, 40, "ppdd", 1.0, 100.0, 16.2, 0, 1.0, 6, 0xFFFFFFFF, name="R32_periodic_x"),
]


@pytest.mark.parametrize("case", GEOMETRY_SETS, ids=[c["name"] for c in GEOMETRY_SETS])
def test_geometry_does_not_change_a_bit(csim, case):
    X = plc.start_state(case)
    M = plc.forecast_members(case)
    auto = perturbed(csim, case, X)
    assert not same_bits(auto, X)
    for tile_rows in (8, 32):
        for shares in (1, 2, 7, M, 65535):
            got = perturbed(csim, case, X, tile_rows, shares)
            assert same_bits(got, auto), f"tile_rows {tile_rows}, shares {shares}: {where_differs(got, auto)}"


def test_options(csim):
    e = csim.Ensemble(3, 8, 8, 1.0, 1.0, (0, 0, 0, 0))
    try:
        assert e.get_option("perturb_tile_rows") == 0 and e.get_option("perturb_member_shares") == 0
        for v in (8, 32, 0):
            e.set_option("perturb_tile_rows", v)
            assert e.get_option("perturb_tile_rows") == v
        for v in (1, 7, 65535, 0):
            e.set_option("perturb_member_shares", v)
            assert e.get_option("perturb_member_shares") == v
        e.set_option("perturb_tile_rows", 32)
        e.set_option("perturb_member_shares", 5)
        for key, bad in (("perturb_tile_rows", (-1, 1, 16, 31, 33, 64)), ("perturb_member_shares", (-1, 65536, 1 << 31))):
            kept = e.get_option(key)
            for v in bad:
                with pytest.raises(csim.CsimError) as ei:
                    e.set_option(key, v)
                assert ei.value.code == 1, (key, v)
                assert e.get_option(key) == kept
    finally:
        e.close()


# ---- c. ping-pong and the chain ---------------------------------------------------------------------------------------

def test_perturb_follows_the_current_buffer_and_chains(csim):
    B, nx, ny, bcs = 5, 70, 45, "pppp"
    bc = csim.bc_codes(bcs)
    X = plc.start_state(dict(B=B, nx=nx, ny=ny, draw=0))
    e = csim.Ensemble(B, nx, ny, 1.0, 0.8, bc, 0.5)
    try:
        e.upload_all(X)
        e.set_physics(0.05, 0.1, 0.5, -0.25)
        e.set_option("fuse", 0)                       # single steps: three steps are three buffer swaps
        e.set_option("perturb_tile_rows", 32)
        e.run(3)
        before = e.download_all()
        assert not same_bits(before, X)
        e.perturb(0.3, 2.0, 5, 1, truth_member=2)
        mid = e.download_all()
        want = ref.perturb(before, 5, 1, 0.3, 2.0, 0, 2, 1.0, 0.8, bc)
        assert same_bits(mid, want), where_differs(mid, want)
        # two more calls with other draws, one centered, no download in between
        e.set_option("perturb_member_shares", 3)
        e.perturb(-0.2, 5.0, 5, 2, centered=True, truth_member=2)
        e.perturb(0.1, 0.0, 5, 3)
        got = e.download_all()
        want = ref.perturb(ref.perturb(mid, 5, 2, -0.2, 5.0, 1, 2, 1.0, 0.8, bc), 5, 3, 0.1, 0.0, 0, None, 1.0, 0.8, bc)
        assert same_bits(got, want), where_differs(got, want)
        assert not same_bits(got[2], mid[2])          # the last call had no truth member
    finally:
        e.close()


# ---- d. the far tail on the device --------------------------------------------------------------------------------------

@pytest.mark.parametrize("ft", plc.FAR_TAIL, ids=[f"seed{ft['seed']}" for ft in plc.FAR_TAIL])
def test_far_tail_of_the_deviate(csim, ft):
    """corr_len 0 on a bounded 64 x 64 grid at unit spacing: taps [1], so on a zero state with sigma = 1 a cell's new
    value is its deviate.  The cell of the case has r = sqrt(-ln t) > 5 (tests/test_ensemble_perturb_launch_host.py)."""
    n, B = plc.FAR_TAIL_N, ft["B"]
    X = np.zeros((B, n + 2, n + 2))
    e = csim.Ensemble(B, n, n, 1.0, 1.0, (0, 0, 0, 0))
    try:
        e.upload_all(X)
        e.perturb(1.0, 0.0, ft["seed"], ft["draw"])
        got = e.download_all()
    finally:
        e.close()
    want = ref.perturb(X, ft["seed"], ft["draw"], 1.0, 0.0, 0, None, 1.0, 1.0, (0, 0, 0, 0))
    assert same_bits(got, want), where_differs(got, want)
    cell = got[ft["member"], ft["row"] + 1, ft["col"] + 1]
    assert cell == ft["value"] and abs(cell) > 6.7
    assert np.abs(got).max() == abs(cell)             # the only deviate of the field that far out
