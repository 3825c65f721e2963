"""What the launch-seam test of csim_ensemble_perturb (tests/test_gpu_ensemble_perturb_seams.py) reaches, checked on
the CPU: its targeted cases and its seeded fuzz are classified by the launch ens_launch_perturb would pick for them
(tests/perturb_launch_cases.py), the 15 older cases of tests/test_gpu_ensemble_perturb.py by the same rule, so that the
gaps the newer file closes stay written down; and the far-tail constants of the device test are pinned to the
library's host function."""
import numpy as np
import pytest

import perturb_launch_cases as plc
import perturb_restatement as ref
from __graft_entry__ import load_package
from test_gpu_ensemble_perturb import CASES as OLD_CASES


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    return pkg


def labels(c):
    """the items of the coverage list that case c reaches"""
    d = plc.describe(c)
    inst = f"<{d['TY']},{int(d['centered'])}>"
    out = {f"instantiation {inst}", f"ty{d['TY']} ny{c['ny']}", f"nx{c['nx']}"}
    if d["lds"] > 65536:
        out.add(f"lds > 64 KiB {inst}")
    if d["lds"] == 147456:
        out.add(f"lds 147456 {inst}")
    if d["auto"]:
        out.add(f"auto {inst} tiles32 {-(-c['nx'] // 64) * -(-c['ny'] // 32)} M {d['M']}")
    if d["tiles_x"] >= 2 and d["last_w"] == 1:
        out.add("last tile one column wide")
    if d["tiles_y"] >= 2 and d["last_h"] == 1:
        out.add(f"last tile one row high ty{d['TY']}")
    if d["px_odd"]:
        out.add(f"odd Px ty{d['TY']}")
    if d["perx"] and c["nx"] & 1 and d["rx"] > 0 and d["tiles_x"] == 3 and d["TY"] == 32 and d["wrap_tiles_x"] == [0, 2]:
        out.add("periodic x, odd nx, three tiles, ty32: wrap in the first and last tile only")
    if d["perx"] and d["rx"] == (c["nx"] - 1) // 2 and d["rx"] > 0:
        out.add("periodic clip in x")
    if d["pery"] and d["ry"] == (c["ny"] - 1) // 2 and d["ry"] > 0:
        out.add("periodic clip in y")
    if d["wrap_y"] and not d["perx"]:
        out.add(f"periodic y only ty{d['TY']}")
    if d["wrap_x"] and not d["pery"]:
        out.add("periodic x only")
    if (d["rx"], d["ry"]) in ((32, 0), (0, 32)):
        out.add(f"radii {d['rx']}, {d['ry']} ty{d['TY']}")
    for p in d["parities"]:
        out.add(f"pair parity {p} ty{d['TY']}")
    if d["shares"] == 1 and d["M"] >= 65:
        out.add(f"one share walks {d['M']} members, centered {int(d['centered'])}")
    if d["shares"] == d["M"] and c["shares"] > 0 and d["M"] > 1:
        out.add("forced shares = M")
    if d["strided"] and d["rem"]:
        out.add(f"strided, M % shares != 0, centered {int(d['centered'])}")
    if d["strided"] and d["shares"] > 1:
        out.add(f"strided with the truth member {d['truth']}")
    if c["sigma"] < 0:
        out.add("negative sigma")
    if c["seed"] >= 1 << 32:
        out.add("seed above 32 bits")
    if c["draw"] >= 1 << 16:
        out.add("draw above 16 bits")
    return out


@pytest.fixture(scope="module")
def reached():
    seam, fuzz = set(), set()
    for c in plc.SEAM_CASES:
        seam |= labels(c)
    for c in plc.fuzz_cases(plc.DEFAULT_SEED):
        fuzz |= labels(c)
    return seam, fuzz


def test_generator_is_a_pure_function_of_the_seed():
    a, b = plc.fuzz_cases(plc.DEFAULT_SEED), plc.fuzz_cases(plc.DEFAULT_SEED)
    assert repr(a) == repr(b) and len(a) == plc.FUZZ_CASES == 60
    assert repr(plc.fuzz_cases(plc.DEFAULT_SEED + 1, 20)) != repr(a[:20])
    assert repr(plc.fuzz_cases(plc.DEFAULT_SEED, 20)) == repr(a[:20])
    names = [c["name"] for c in plc.SEAM_CASES + a]
    assert len(set(names)) == len(names)


def test_no_case_can_be_refused(csim):
    """every radius is at most PERTURB_MAX_RADIUS and every argument is one csim_ensemble_perturb accepts; over several
    seeds, since this is a property of the generator"""
    assert csim.PERTURB_MAX_RADIUS == plc.MAX_RADIUS
    cases = plc.SEAM_CASES + [c for s in range(5) for c in plc.fuzz_cases(plc.DEFAULT_SEED + s)]
    for c in cases:
        d = plc.describe(c)
        assert 0 <= d["rx"] <= plc.MAX_RADIUS and 0 <= d["ry"] <= plc.MAX_RADIUS, c["name"]
        assert d["M"] >= (2 if c["centered"] else 1), c["name"]
        assert c["t"] is None or 0 <= c["t"] < c["B"], c["name"]
        assert c["sigma"] != 0 and np.isfinite(c["sigma"]) and c["corr_len"] >= 0, c["name"]
        assert 0 <= c["seed"] < 1 << 64 and 0 <= c["draw"] < 1 << 32, c["name"]
        assert c["tile_rows"] in (0, 8, 32) and 0 <= c["shares"] <= 65535, c["name"]
        assert d["lds"] <= 160 * 1024 and 1 <= d["shares"] <= min(d["M"], 65535), c["name"]
    for c in plc.fuzz_cases(plc.DEFAULT_SEED):
        assert 1 <= c["nx"] <= 200 and 1 <= c["ny"] <= 100 and 1 <= c["B"] <= 40
        # the library's own radius, through its taps
        for d_, n, per, want in ((c["dx"], c["nx"], 0, "rx"), (c["dy"], c["ny"], 1, "ry")):
            periodic = ref.axis_periodic(plc.bc_codes(c["bc"]))[per]
            assert len(csim.ensemble_perturb_taps(d_, c["corr_len"], n, periodic)) == 2 * plc.describe(c)[want] + 1


def test_launch_choice_without_options_is_the_documented_heuristic():
    assert plc.launch_choice(130, 67, 113, False) == (8, 76)      # 9 * 113 = 1017 < 1024: 27 tiles of 8 rows
    assert plc.launch_choice(130, 67, 114, False) == (32, 114)    # 1026
    assert plc.launch_choice(1024, 480, 2, True) == (8, 1)        # 240 tiles of 32 rows
    assert plc.launch_choice(1024, 512, 2, True) == (32, 2)       # 256
    assert plc.launch_choice(130, 67, 9, False, 32, 0) == (32, 9)
    assert plc.launch_choice(130, 67, 9, False, 8, 65535) == (8, 9)
    assert plc.launch_choice(130, 67, 9, True, 0, 7) == (8, 7)


def test_lds_of_every_instantiation(reached):
    seam, _ = reached
    for inst in ("<8,0>", "<8,1>", "<32,0>", "<32,1>"):
        assert f"lds > 64 KiB {inst}" in seam, inst
    assert "lds 147456 <32,0>" in seam and "lds 147456 <32,1>" in seam
    assert max(plc.describe(c)["lds"] for c in plc.SEAM_CASES) == 147456 == 8 * (32 + 64) * (128 + 64)


def test_both_sides_of_the_automatic_seam(reached):
    seam, _ = reached
    for item in ("auto <8,0> tiles32 9 M 113", "auto <32,0> tiles32 9 M 114", "auto <8,1> tiles32 240 M 2",
                 "auto <32,1> tiles32 256 M 2"):
        assert item in seam, item


def test_tile_edges(reached):
    seam, _ = reached
    for nx in (63, 64, 65, 128, 129):
        assert f"nx{nx}" in seam, nx
    for ty in (8, 32):
        for ny in (7, 8, 9, 31, 32, 33):
            assert f"ty{ty} ny{ny}" in seam, (ty, ny)
        assert f"last tile one row high ty{ty}" in seam
    assert "last tile one column wide" in seam


def test_wraps_parities_and_radii(reached):
    seam, fuzz = reached
    for item in ("periodic x, odd nx, three tiles, ty32: wrap in the first and last tile only", "periodic clip in x",
                 "periodic clip in y", "periodic y only ty8", "periodic y only ty32", "periodic x only", "odd Px ty8",
                 "odd Px ty32", "radii 32, 0 ty8", "radii 32, 0 ty32", "radii 0, 32 ty8", "radii 0, 32 ty32",
                 "pair parity 0 ty8", "pair parity 1 ty8", "pair parity 0 ty32", "pair parity 1 ty32"):
        assert item in seam, item
    for item in ("odd Px ty8", "odd Px ty32", "pair parity 1 ty8", "pair parity 1 ty32", "negative sigma",
                 "seed above 32 bits", "draw above 16 bits"):
        assert item in fuzz, item


def test_member_shares(reached):
    seam, fuzz = reached
    for item in ("one share walks 65 members, centered 0", "one share walks 65 members, centered 1",
                 "forced shares = M", "strided, M % shares != 0, centered 0", "strided, M % shares != 0, centered 1",
                 "strided with the truth member first", "strided with the truth member middle",
                 "strided with the truth member last", "strided with the truth member absent"):
        assert item in seam, item
    for inst in ("<8,0>", "<8,1>", "<32,0>", "<32,1>"):
        assert f"instantiation {inst}" in fuzz, inst
    for where in ("first", "middle", "last", "absent"):
        assert f"strided with the truth member {where}" in fuzz, where


def test_the_gaps_of_the_older_cases():
    """the launch of each of the 15 cases of tests/test_gpu_ensemble_perturb.py, and what none of them reaches"""
    assert len(OLD_CASES) == 15
    ds = [plc.describe(plc.from_tuple(t)) for t in OLD_CASES]
    got = {(t[0], t[2], t[3], t[4], t[8]): (d["rx"], d["ry"], d["TY"], d["shares"], d["M"], d["lds"])
           for t, d in zip(OLD_CASES, ds)}
    table = {(9, 130, 67, "nnnn", 0): (32, 32, 8, 8, 8, 110592),
             (3, 67, 130, "pppp", 1): (15, 15, 8, 2, 2, 48032),
             (65, 300, 261, "dddd", 0): (6, 5, 32, 46, 64, 47040),
             (9, 512, 512, "pppp", 0): (3, 3, 32, 9, 9, 40736),
             (3, 1024, 520, "ddpp", 1): (1, 1, 32, 2, 3, 35360)}
    for key, want in table.items():
        assert got.pop(key) == want, key
    assert len(got) == 10
    for key, (rx, ry, TY, shares, M, lds) in got.items():
        assert TY == 8 and max(rx, ry) <= 6 and lds <= 21760, key
    old = set()
    for t in OLD_CASES:
        old |= labels(plc.from_tuple(t))
    # 1. only <8, false> above 64 KiB; the largest launch never; 32-row tiles only with radii up to 6
    assert {s for s in old if s.startswith("lds")} == {"lds > 64 KiB <8,0>"}
    assert max(max(d["rx"], d["ry"]) for d in ds if d["TY"] == 32) == 6
    # 3. neither side of either switch: uncentered, tiles32 * M is 640 at most below 1024 and 1152 at least above it;
    # centered, tiles32 is 128 below 256 and 272 above it
    prod = sorted(-(-t[2] // 64) * -(-t[3] // 32) * d["M"] for t, d in zip(OLD_CASES, ds) if not d["centered"])
    assert max(p for p in prod if p < 1024) == 640 and min(p for p in prod if p >= 1024) == 1152
    cen = sorted(-(-t[2] // 64) * -(-t[3] // 32) for t, d in zip(OLD_CASES, ds) if d["centered"])
    assert max(p for p in cen if p < 256) == 128 and min(p for p in cen if p >= 256) == 272
    # 4. parities, wraps, anisotropy, thin last tiles
    assert "odd Px ty8" in old and "odd Px ty32" not in old
    assert "periodic x, odd nx, three tiles, ty32: wrap in the first and last tile only" not in old
    assert not {s for s in old if s.startswith("radii")}
    # (12 x 9 has a last tile one row high under 8-row tiles; nothing has one under 32-row tiles or one column wide)
    assert {s for s in old if s.startswith("last tile one")} == {"last tile one row high ty8"}
    assert all(d["auto"] for d in ds)


def test_far_tail_constants(csim):
    """the two cells of the device test: r = sqrt(-ln t) > 5 in the restatement, and the library's host function gives
    the restatement's bits for the same 64 random bits"""
    for ft in plc.FAR_TAIL:
        bits = plc.far_tail_bits(ft)
        u = ref.uniform_from_bits(bits)
        t = np.atleast_1d(np.where(u < 0.5, u, 1.0 - u))
        r = float(np.sqrt(-ref.log_restated(t))[0])
        assert r > 5.0 and abs(r - ft["r"]) < 5e-5, (ft, r)
        want = ref.normal_from_bits(bits)
        got = csim.normal_from_bits(np.array([bits], dtype=np.uint64))
        assert np.array_equal(np.asarray(got).view(np.int64), want.view(np.int64))
        assert float(want[0]) == ft["value"]
        L = np.array([ft["row"] * plc.FAR_TAIL_N + ft["col"]], dtype=np.uint64)
        assert float(ref.white(ft["seed"], ft["draw"], ft["member"], L)[0]) == ft["value"]
        assert ft["member"] < ft["B"]
    assert plc.FAR_TAIL[0]["value"] < -6.85 and plc.FAR_TAIL[1]["value"] > 6.73
    assert int(plc.far_tail_bits(plc.FAR_TAIL[0])) >> 12 == 16496
