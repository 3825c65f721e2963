"""The wide-strip sweep as the benchmark launches it.  tests/test_gpu_wide_strip.py forces "wide_strips" = 1 on fields
of at most 1100 x 64 cells: chunks of 6 or 11 rows (three groups of six per march), no tail, at most five tile regions.
The launch bench.py times is another one: 16384^2 with default options takes wide strips ("wide_strips" = 2) once a pass
is handed a verdict word, in 66-row chunks (13 groups of six), with a tail region at half height and so all eight
regions of Tiling::r[8] — the last iteration of the kernel's region decode — and with the wide kernel's own chunk-height
trial (tune_rows with cfg.wide), which needs 2^22 cells.  Here:
  (a) the timed configuration at the flagship shape against the oracle's committed checksum, the lease arriving in the
      first fused pass or in the middle of the last call;
  (b) the two smallest wide plans that have a tail, against the oracle, bit for bit;
  (c) chunks of 18, 66 and 236 rows at a small shape: the long march of the four-column bodies;
  (d) the wide kernel's trial at the smallest field that has one.
Which plan a launch took is read back through "last_regions", "last_tiles", "last_tail_blocks" and asserted, so that a
test cannot pass by having run a simpler launch; tests/test_sweep_plan_shapes_host.py pins the same tables on the CPU.
Every comparison is of bits (NaN positions included, ghost ring included) or of the 64-bit checksum."""
import json
import os

import numpy as np
import pytest

from oracle import cpu_oracle as ora
from test_gpu_wide_strip import BASE, D, DT, assert_bits, csim, geometry  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VX, VY = 0.5, 0.25
BODIES = {"leased_p2": 3, "negative": 1, "unleased": 0}   # body -> the verdict word a Dirichlet ring of zeros leaves
READBACK = ("lease_reductions", "wide_strips_active", "last_rows", "last_regions", "last_tiles", "last_tail_blocks",
            "tuned_rows", "tuned_rows_6", "tuned_rows_7", "tuned_rows_wide_6", "tuned_rows_wide_7")


def whole_groups(T, rows):
    """sweep_plan.hpp: rows rounded up so that rows + 2 (T - 1) is a multiple of six"""
    return rows + (6 - (rows + 2 * (T - 1)) % 6) % 6


def band(T):
    return whole_groups(T, T - 1)


def trial_candidates(T, ny):
    """the chunk heights tune_rows (csrc/passes.cpp) times: its ladder 6, 10, .. 30, 36, .. 234, snapped to whole groups"""
    cand, ry = [], 6
    while ry <= 236 and ry <= ny:
        snapped = whole_groups(T, ry)
        if snapped <= ny and (not cand or cand[-1] != snapped):
            cand.append(snapped)
        ry += 4 if ry < 30 else 6
    return cand


def readback(st):
    return {k: st.get_option(k) for k in READBACK}


def varying(nx, ny):
    """a strictly positive field no two neighbouring cells of which are equal, in a row or in a column (checked): a tile
    that loaded the wrong rows or columns of it cannot go unnoticed, as it could on the flat background of a hotspot"""
    i, j = np.arange(nx + 2, dtype=np.float64), np.arange(ny + 2, dtype=np.float64)
    u = 0.5 + 0.25 * np.outer(np.cos(0.7548776662466927 * j + 0.7), np.sin(1.4142135623730951 * i + 0.3))
    s = 0.08 * nx
    u += np.outer(np.exp(-(j - 0.55 * ny) ** 2 / (2.0 * s * s)), np.exp(-(i - 0.4 * nx) ** 2 / (2.0 * s * s)))
    inner = u[1:-1, 1:-1]
    assert inner.min() >= 0.25
    assert (inner[:, 1:] != inner[:, :-1]).all() and (inner[1:, :] != inner[:-1, :]).all()
    u[0, :] = u[-1, :] = u[:, 0] = u[:, -1] = 0.0
    return u


def with_body(base, body, cell):
    """the three bodies of tests/test_gpu_wide_strip.py, the offending cells placed at `cell` (row, column)"""
    u0 = base.copy()
    r, c = cell
    if body == "negative":
        u0[r, c] = -0.5
    elif body == "unleased":
        u0[r:r + 2, c:c + 3] = 1e300
        u0[r + 3, c + 40:c + 42] = np.nan
    return u0


def oracle_world(u0, steps, bc):
    """the oracle on 16 tiles and 16 threads (as tests/test_gpu_bench.py runs it): the whole array, ghost ring included"""
    ny, nx = u0.shape[0] - 2, u0.shape[1] - 2
    w = ora.World(16, nx, ny)
    w.scatter(np.ascontiguousarray(u0[1:-1, 1:-1]))
    w.run(D, VX, VY, DT, ora.bc_codes(bc), steps, threads=16)
    want = w.gather_full()
    want.setflags(write=False)
    return want


@pytest.fixture(scope="module")
def cache():
    """base fields and oracle results per (shape, body, steps, bc): computed once, read-only, given back with the module"""
    c = {}
    yield c
    c.clear()


def stepper(csim, nx, ny, bc, opts):
    st = csim.Stepper.single(nx, ny, 1.0, 1.0, csim.bc_codes(bc), 0.0)
    for k, v in opts.items():
        st.set_option(k, v)
    return st


def test_plan_readback_is_read_only_and_follows_the_launch(csim):
    """"last_regions", "last_tiles", "last_tail_blocks": 0 before any fused launch, the plan of the last whole-field one
    afterwards (360 x 30 at T = 7: left, one wide, right strips of three 6-row chunks, two bands of four strips), and
    not to be set"""
    st = stepper(csim, 360, 30, "dddd", {**BASE, "fuse": 7})
    for k in ("last_regions", "last_tiles", "last_tail_blocks"):
        assert st.get_option(k) == 0
        with pytest.raises(csim.CsimError, match=k + " is read-only"):
            st.set_option(k, 1)
    st.upload(varying(360, 30))
    st.run(D, DT, VX, VY, 1)   # a single step plans no tiles
    assert [st.get_option(k) for k in ("last_regions", "last_tiles", "last_tail_blocks")] == [0, 0, 0]
    st.run(D, DT, VX, VY, 7)
    assert [st.get_option(k) for k in ("last_regions", "last_tiles", "last_tail_blocks")] == [5, 17, 2]
    st.set_option("wide_strips", 0)
    st.run(D, DT, VX, VY, 7)
    assert [st.get_option(k) for k in ("last_regions", "last_tiles", "last_tail_blocks")] == [3, 20, 2]
    st.close()


# ---- (a) ------------------------------------------------------------------------------------------------------------
N = 16384
FLAGSHIP = dict(regions=8, tiles=19544, tail_blocks=1106, rows=66)   # the untuned wide plan at T = 7 (sweep_plan.cpp)
FLAGSHIP_NARROW = dict(regions=4, tiles=40719, tail_blocks=2242, rows=66)


def fixture_entry(bc):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "bench_checksum.json")))["entries"]
    (e,) = [x for x in fx if (x["nx"], x["ny"], x["bc"], x["vx"], x["vy"], x["steps"]) == (N, N, bc, VX, VY, 40)]
    return e


def run_fixture_calls(st, e, log=None):
    st.init_gaussian(1.0, 0.05, 0.5, 0.5)
    for n in (1, 7, 32):
        st.run(e["D"], e["dt"], e["vx"], e["vy"], n)
        if log is not None:
            log.append(readback(st))
    return st.checksum()


def default_after_8(csim, cache, e):
    """checksum of a fresh default stepper (no lease before step 512: the narrow, screened kernel) after 1 + 7 steps"""
    key = ("default_after_8", e["bc"])
    if key not in cache:
        st = stepper(csim, N, N, e["bc"], {})
        st.init_gaussian(1.0, 0.05, 0.5, 0.5)
        for n in (1, 7):
            st.run(e["D"], e["dt"], e["vx"], e["vy"], n)
        assert (st.get_option("wide_strips_active"), st.get_option("lease_reductions")) == (0, 0)
        cache[key] = st.checksum()
        st.close()
    return cache[key]


def diagnose(st, e, got, log):
    """a checksum gives no location: say what was launched, and whether the same stepper without wide strips matches —
    which points at the wide launch, or else at the lease"""
    st.set_option("wide_strips", 0)
    narrow = run_fixture_calls(st, e)
    opts = {k: st.get_option(k) for k in ("wide_strips", "pow2_v", "screen_lease", "lease_steps", "lease_acquire_after", "fuse")}
    return (f"checksum {got:#x}, the oracle's {e['checksum']:#x} ({e['bc']}); after each call: {log}; options {opts}; "
            f"the same stepper with wide_strips = 0: {narrow:#x}, "
            f"{'matches: look at the wide launch' if narrow == e['checksum'] else 'differs too: look at the lease'}")


@pytest.mark.parametrize("acquire_after", [0, 14])
@pytest.mark.parametrize("bc", ["dddd", "nnnn", "dnpd"])
def test_flagship_launch_matches_the_oracle_checksum(csim, cache, bc, acquire_after):
    """16384^2, default options but "lease_acquire_after", 1 + 7 + 32 steps of the device-made hotspot, against the
    oracle's checksum in tests/golden/bench_checksum.json.  What the three calls launch, derived from csim_stepper_run,
    pass_fused, lease_for_pass, launch_cfg and tune_rows (csrc/passes.cpp) — depth 7 is preferred at this size, the pass
    plans are [1], [7] and [7, 7, 6, 6, 6] — and asserted below through the read-only options after every call:

    "lease_acquire_after" = 0
      run(1)   one single-step pass; the lease is untouched (lease_for_pass is called by fused passes only), idle = 1
      run(7)   7 < 4 x 7: no trial.  The pass is not yet tuned, so no wide trial either; lease_for_pass acquires (0 >= 0:
               reduction 1) and the launch is the WIDE kernel at T = 7 on the untuned plan: 66-row chunks, 8 regions,
               19544 tiles, 1106 tail blocks
      run(32)  32 >= 28 and nothing tuned: run()'s own trial, and since a lease is held it times the WIDE kernel at T = 7
               (tuned_rows_wide_7; tuned_rows_7 stays 0).  Passes 7, 7 wide at that height; in front of the first pass
               of depth 6 pass_fused runs the wide trial for T = 6 between two passes of the run, under the lease
               (tuned_rows_wide_6); passes 6, 6, 6 wide at that height.  One reduction in all
    "lease_acquire_after" = 14
      run(1)   as above, idle = 1
      run(7)   idle 1 < 14: no word, so "wide_strips" = 2 keeps the NARROW screened kernel: 4 regions, 40719 tiles; idle = 8
      run(32)  run()'s trial has no lease and times the narrow kernel at T = 7 (tuned_rows_7).  Pass 1 (7): idle 8 < 14,
               narrow.  Pass 2 (7): pass_fused looks for a held lease BEFORE lease_for_pass acquires one, finds none, so no
               wide trial; then idle 15 >= 14: reduction 1, and the launch is the wide kernel at T = 7 at the NARROW
               kernel's tuned height (tuned_rows_wide_7 stays 0: the one wide launch of depth 7 had no trial of its own).
               Pass 3 (6): the lease is held, so pass_fused runs the wide trial for T = 6 (tuned_rows_wide_6) between
               two passes; passes 6, 6, 6 wide.  tuned_rows_6 stays 0: no narrow launch of depth 6
    Afterwards the same stepper is given a new field, whose verdict word must read 0, and runs 1 + 7 steps: with 14 no
    pass is handed a word (narrow, no further reduction); with 0 the first fused pass acquires at once (wide, a second
    reduction).  Either way the checksum is that of a fresh default stepper after the same steps."""
    e = fixture_entry(bc)
    assert csim.pass_schedule(7, tile_cells=N * N) == [7] and csim.pass_schedule(32, tile_cells=N * N) == [7, 7, 6, 6, 6]
    st = stepper(csim, N, N, bc, dict(lease_acquire_after=acquire_after))
    log = []
    got = run_fixture_calls(st, e, log)
    word = st.get_option("lease_word")
    print(f"flagship {bc} lease_acquire_after={acquire_after}: word {word}, after each call {log}")
    if got != e["checksum"]:
        pytest.fail(diagnose(st, e, got, log))
    one, seven, last = log
    assert (one["lease_reductions"], one["wide_strips_active"]) == (0, 0), log

    def plan_of(rec):
        return dict(regions=rec["last_regions"], tiles=rec["last_tiles"], tail_blocks=rec["last_tail_blocks"], rows=rec["last_rows"])

    untuned = dict(tuned_rows=0, tuned_rows_6=0, tuned_rows_7=0, tuned_rows_wide_6=0, tuned_rows_wide_7=0)
    assert {k: seven[k] for k in untuned} == untuned, log
    if acquire_after == 0:
        assert (seven["lease_reductions"], seven["wide_strips_active"]) == (1, 1) and plan_of(seven) == FLAGSHIP, log
        assert last["tuned_rows_wide_7"] in trial_candidates(7, N) and last["tuned_rows_7"] == 0, log
        assert last["tuned_rows"] == last["tuned_rows_wide_7"], log
    else:
        assert (seven["lease_reductions"], seven["wide_strips_active"]) == (0, 0) and plan_of(seven) == FLAGSHIP_NARROW, log
        assert last["tuned_rows_7"] in trial_candidates(7, N) and last["tuned_rows_wide_7"] == 0, log
        assert last["tuned_rows"] == last["tuned_rows_7"], log
    assert last["wide_strips_active"] == 1 and last["lease_reductions"] == 1, log
    assert last["tuned_rows_wide_6"] in trial_candidates(6, N) and last["tuned_rows_6"] == 0, log
    assert last["last_rows"] == last["tuned_rows_wide_6"], log   # the last launch: depth 6, wide, at its own trial's height
    # (a tail needs chunks of at least 48 rows; the wide trial's choices at this size lie between 116 and 212:
    # profiles/wide_strip_ab.jsonl.  The untuned plan of run(7) above does not depend on a trial.)
    assert last["last_regions"] == 8 and last["last_tail_blocks"] > 0, log
    if bc == "dddd":
        assert word == 3
    # a new field on the same stepper
    st.init_gaussian(1.0, 0.05, 0.5, 0.5)
    assert st.get_option("lease_word") == 0
    for n in (1, 7):
        st.run(e["D"], e["dt"], e["vx"], e["vy"], n)
    again = readback(st)
    assert (again["wide_strips_active"], again["lease_reductions"]) == ((1, 2) if acquire_after == 0 else (0, 1)), again
    assert st.checksum() == default_after_8(csim, cache, e), again
    st.close()


def test_flagship_launch_without_wide_strips(csim):
    """"wide_strips" = 0 with the lease from the first fused pass on: the leased narrow kernel, the same checksum"""
    e = fixture_entry("dddd")
    st = stepper(csim, N, N, "dddd", dict(wide_strips=0, lease_acquire_after=0))
    log = []
    got = run_fixture_calls(st, e, log)
    assert got == e["checksum"], (hex(got), log)
    assert [rec["wide_strips_active"] for rec in log] == [0, 0, 0] and log[-1]["lease_reductions"] == 1, log
    assert log[-1]["tuned_rows_wide_6"] == 0 and log[-1]["tuned_rows_wide_7"] == 0, log
    assert st.get_option("lease_word") == 3
    st.close()


# ---- (b) ------------------------------------------------------------------------------------------------------------
# shape -> T, regions, tiles, tail blocks, the tail's chunk height (tests/test_sweep_plan_shapes_host.py has the tables)
TAIL_SHAPES = {(600, 49181): (7, 8, 4624, 260, 24), (618, 49179): (6, 8, 4544, 240, 26)}
TAIL_CELL = (46003, 200)   # row, column of the offending cells: in the first wide strip of the TAIL region of both shapes
                           # (rows 43015 / 43017 up, output columns 112 / 116 .. 351 / 359)


@pytest.mark.parametrize("shape,body", [((600, 49181), "leased_p2"), ((600, 49181), "negative"), ((600, 49181), "unleased"),
                                        ((618, 49179), "leased_p2")])
def test_smallest_wide_plans_with_a_tail_match_the_oracle(csim, cache, shape, body):
    """all eight regions, two wide strips per row, 48-row chunks and a tail of half-height chunks whose last one is
    ragged; the offending cells of the refused bodies sit in a wide tile of the tail"""
    nx, ny = shape
    T, regions, tiles, tail_blocks, half = TAIL_SHAPES[shape]
    assert half == whole_groups(T, 24) and 112 <= TAIL_CELL[1] - 1 and TAIL_CELL[1] + 42 <= 351
    assert ny - band(T) - TAIL_CELL[0] > 2 * T + 8 and TAIL_CELL[0] > 43017 + 2 * T + 8   # well inside the tail's rows
    if ("base", shape) not in cache:
        cache[("base", shape)] = varying(nx, ny)
    u0 = with_body(cache[("base", shape)], body, TAIL_CELL)
    steps = 1 + 2 * T
    key = (shape, body, steps, "dddd")
    if key not in cache:
        cache[key] = oracle_world(u0, steps, "dddd")
    st = stepper(csim, nx, ny, "dddd", {**BASE, "fuse": T, "rows_per_chunk": 48})
    st.upload(u0)
    st.run(D, DT, VX, VY, 1)
    st.run(D, DT, VX, VY, 2 * T)   # a fixed depth is balanced over the passes of a call: two passes of exactly T
    rec, word = readback(st), st.get_option("lease_word")
    got = st.download()
    st.close()
    assert rec["wide_strips_active"] == 1 and rec["last_rows"] == 48, rec
    assert (rec["last_regions"], rec["last_tiles"], rec["last_tail_blocks"]) == (regions, tiles, tail_blocks), rec
    assert word == BODIES[body]
    assert_bits(got, cache[key], (shape, T, body, rec))


# ---- (c) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", list(BODIES))
@pytest.mark.parametrize("T", [6, 7])
@pytest.mark.parametrize("rows", [18, 66, 236])
def test_tall_chunks_at_a_small_shape(csim, cache, rows, T, body):
    """849 columns, two chunks of `rows` rows and a ragged third of 7 between the bands: 18 rows are the default minimum,
    66 the flagship's height, 236 the trial's largest candidate — 5, 13 and 41 or 42 groups of six per march, where the
    shapes of tests/test_gpu_wide_strip.py stop at three (the two start-up copies of the group and ONE steady one)"""
    nx, ny = 849, 2 * band(T) + 2 * rows + 7
    s2, s4, tp = geometry(T)
    nwide = (nx - tp - s2) // s4
    nright, nstrips = -(-(nx - s2 - nwide * s4) // s2), -(-nx // s2)
    cell = (band(T) + rows, 200)   # the last row of the first chunk: the patches reach into the second
    if ("base", nx, ny) not in cache:
        cache[("base", nx, ny)] = varying(nx, ny)
    u0 = with_body(cache[("base", nx, ny)], body, cell)
    steps = 1 + 2 * T
    for bc in ("dddd", "nnnn"):
        key = ((nx, ny), body, steps, bc)
        if key not in cache:
            w = u0.copy()
            with np.errstate(all="ignore"):
                ora.run_single(w, 1.0, 1.0, D, VX, VY, DT, ora.bc_codes(bc), steps, 0.0)
            w.setflags(write=False)
            cache[key] = w
        st = stepper(csim, nx, ny, bc, {**BASE, "fuse": T, "rows_per_chunk": rows})
        st.upload(u0)
        st.run(D, DT, VX, VY, 1)
        st.run(D, DT, VX, VY, 2 * T)
        rec, word = readback(st), st.get_option("lease_word")
        got = st.download()
        st.close()
        assert rec["wide_strips_active"] == 1 and rec["last_rows"] == rows, rec
        # left, wide, right (three chunks each) and the two bands; too few chunks for a tail
        assert (rec["last_regions"], rec["last_tiles"]) == (5, 3 * (1 + nwide + nright) + 2 * nstrips), rec
        if bc == "dddd":
            assert word == BODIES[body]
        assert_bits(got, cache[key], (rows, T, body, bc, rec))


# ---- (d) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", ["leased_p2", "unleased"])
def test_wide_trial_at_the_smallest_field_that_has_one(csim, cache, body):
    """2048^2 is exactly the 2^22 cells tune_rows asks for.  "wide_strips" = 1 offers wide strips with or without a word,
    so the trial run(28) starts with (28 >= 4 x 7, nothing tuned) times the WIDE kernel — before the field's first
    reduction, on the reference's own sequence — and keeps its result apart from the narrow one; the four passes of 7 then
    launch at that height under the lease the first of them acquires.  Trial launches go cur -> nxt without a swap: the
    field must come out as if there had been none."""
    n, T = 2048, 7
    if ("base", n, n) not in cache:
        cache[("base", n, n)] = varying(n, n)
    u0 = with_body(cache[("base", n, n)], body, (1000, 200))
    key = ((n, n), body, 29, "dddd")
    if key not in cache:
        cache[key] = oracle_world(u0, 29, "dddd")
    st = stepper(csim, n, n, "dddd", {**BASE, "fuse": T, "rows_per_chunk": 0, "autotune": 1})
    st.upload(u0)
    st.run(D, DT, VX, VY, 1)
    st.run(D, DT, VX, VY, 28)
    rec, word = readback(st), st.get_option("lease_word")
    got = st.download()
    assert rec["tuned_rows_wide_7"] in trial_candidates(T, n), rec
    assert rec["last_rows"] == rec["tuned_rows_wide_7"] and rec["tuned_rows_7"] == 0, rec
    assert rec["wide_strips_active"] == 1 and rec["lease_reductions"] == 1 and word == BODIES[body], (rec, word)
    assert_bits(got, cache[key], ("wide", body, rec))
    # another kernel: what was tuned is forgotten, and the narrow launches (with a trial of their own) give the same bits
    st.set_option("wide_strips", 0)
    assert st.get_option("tuned_rows_wide_7") == 0
    st.upload(u0)
    st.run(D, DT, VX, VY, 29)
    rec = readback(st)
    got = st.download()
    st.close()
    assert rec["wide_strips_active"] == 0 and rec["tuned_rows_wide_7"] == 0, rec
    assert_bits(got, cache[key], ("narrow", body, rec))
