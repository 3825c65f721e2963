"""The DEFAULT exchange schedule of the multi-rank stepper — "overlap" = 5: bulk launch first, this pass's exchange under
it, and the stream relay ("relay" = 1: the field state hops between two extra streams from pass to pass, every other
entry point brings it back onto the compute stream first) — on ONE GPU with the self-linked torus of
tests/test_gpu_comm.py: its option matrix, every entry point directly behind a relay run (no sync in between),
schedules changed on a live stepper, what the timers count, and the fold of the profiling-event pool in the middle
of a run.  The reference everywhere is the CPU oracle stepping the wrapped tile (torus_oracle); every comparison of
a field is exact on the full array, ghost ring included, corners excepted; every launch count is compared
with the planner's host arithmetic (csim_pass_schedule_for), never with a number read off the library."""
import math
import zlib

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cpu_oracle as ora
from test_gpu_comm import CORNERLESS, self_neighbor_decomp, torus_oracle

pytestmark = pytest.mark.gpu

D, VX, VY, DT = 0.05, 0.5, -0.25, 0.1
ERR_STATE = 4   # CSIM_ERR_STATE (include/csim.h)

# tiles large enough for the frame / bulk split, fully linked and with linked sides next to physical Neumann and
# Periodic sides, and one tile that is all frame (two rows: passes of depth 2 at most)
GEOMS = {
    "torus_1160x300": (1160, 300, (1, 1, 1, 1), "dddd"),
    "leftright_1160x300_ddnp": (1160, 300, (1, 1, 0, 0), "ddnp"),
    "bottomtop_1024x300_pndd": (1024, 300, (0, 0, 1, 1), "pndd"),
    "torus_128x2": (128, 2, (1, 1, 1, 1), "dddd"),
}


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    pkg.set_device(0)
    return pkg


class Case:
    """one geometry: its seeded fields (random interior, random non-zero ghost lines) and the oracle's states of them,
    kept per step count — the oracle does not depend on any option, so every test of a geometry shares them."""

    def __init__(self, csim, name):
        self.name = name
        self.nx, self.ny, self.sides, bc = GEOMS[name]
        self.codes = csim.bc_codes(bc)
        self.mask = CORNERLESS(self.ny, self.nx)
        self.smallest = min(self.nx, self.ny)
        self._states = {}

    def field(self, key=0):
        if key not in self._states:
            rng = np.random.default_rng([zlib.crc32(self.name.encode()), key])
            u0 = rng.standard_normal((self.ny + 2, self.nx + 2))   # ghost lines (and corners) included
            self._states[key] = {0: u0}
        return self._states[key][0]

    def advance(self, u, steps):
        """the oracle's torus, `steps` further steps from the full array `u` (a step rebuilds its ghosts from the
        interior and copies the ring along, so runs compose)"""
        return torus_oracle(u, 1.0, 1.0, D, VX, VY, DT, steps, self.sides, self.codes) if steps else u

    def want(self, steps, key=0):
        self.field(key)
        known = self._states[key]
        if steps not in known:
            base = max(s for s in known if s <= steps)
            known[steps] = self.advance(known[base], steps - base)
        return known[steps]

    def stepper(self, csim):
        st = csim.Stepper(self_neighbor_decomp(csim, self.nx, self.ny, self.sides), 1.0, 1.0, self.codes)
        st.comm_init(csim.comm_unique_id())
        return st

    def same(self, got, want):
        return np.array_equal(got[self.mask], want[self.mask])


_CASES = {}


def case(csim, name):
    if name not in _CASES:
        _CASES[name] = Case(csim, name)
    return _CASES[name]


def run(st, steps):
    st.run(D, DT, VX, VY, steps)


def steps_for(csim, passes, fuse, smallest):
    """the longest run the planner cuts into exactly `passes` passes, none of them a single step"""
    for steps in range(7 * passes, 1, -1):
        depths = csim.pass_schedule(steps, smallest, fuse)
        if len(depths) == passes and min(depths) >= 2:
            return steps
    raise AssertionError((passes, fuse, smallest))


def set_overlap(csim, st, k):
    """a completed run() leaves nothing in flight, so the schedule may change; the one refusal by design is
    schedule 3 on a device without signal memory (CSIM_ERR_STATE), which leaves the schedule as it was"""
    assert st.get_option("faces_in_flight") == 0
    try:
        st.set_option("overlap", k)
    except csim.CsimError as e:
        assert k == 3 and e.code == ERR_STATE and "signal memory" in str(e), e
        return False
    assert st.get_option("overlap") == k
    return True


# ---- a. the relay's option matrix ----------------------------------------------------------------------------
@pytest.mark.parametrize("relay_events", [0, 1])
@pytest.mark.parametrize("relay", [1, 0])
@pytest.mark.parametrize("overlap", [4, 5])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_relay_option_matrix(csim, geom, overlap, relay, relay_events):
    """bulk-first schedules 4 and 5 with and without the relay, with default and light hand-off events, at automatic
    depth and depths 6, 7 and 2: calls of one, two and three passes — the state ends on one relay stream or the other
    by the parity of the passes since the last hand-over — cut into two and into three run() calls."""
    c = case(csim, geom)
    st = c.stepper(csim)
    for k, v in (("overlap", overlap), ("relay", relay), ("relay_events", relay_events)):
        st.set_option(k, v)
        assert st.get_option(k) == v
    for fuse in (-1, 6, 7, 2):
        st.set_option("fuse", fuse)
        assert st.get_option("fuse") == fuse
        for cut in ((1, 2), (2, 1), (3, 1), (1, 1, 1), (2, 3, 1), (3, 2, 2)):
            st.upload(c.field())
            total = 0
            for passes in cut:
                n = steps_for(csim, passes, fuse, c.smallest)
                run(st, n)
                total += n
            got = st.download()
            assert c.same(got, c.want(total)), (fuse, cut, total, int((got != c.want(total))[c.mask].sum()))
    st.close()


# ---- b. every entry point directly after a relay run ---------------------------------------------------------
def _wrapped(c, u):
    """what exchange_halos leaves: the ghost lines of the linked sides hold the opposite edge's cells"""
    w = u.copy()
    if c.sides[0]:
        w[1:-1, 0] = u[1:-1, -2]
    if c.sides[1]:
        w[1:-1, -1] = u[1:-1, 1]
    if c.sides[2]:
        w[0, 1:-1] = u[-2, 1:-1]
    if c.sides[3]:
        w[-1, 1:-1] = u[1, 1:-1]
    return w


def _faces(u, H):
    """k_halo2_pack's layout: the H outermost interior columns over rows 0..ny+1 (column-major), the H outermost
    interior rows over columns 0..nx+1, the H x H corner blocks of interior cells; directions L R B T BL BR TL TR"""
    ny, nx = u.shape[0] - 2, u.shape[1] - 2
    lo, hx, hy = slice(1, 1 + H), slice(nx - H + 1, nx + 1), slice(ny - H + 1, ny + 1)
    return [u[:, lo].T.ravel(), u[:, hx].T.ravel(), u[lo, :].ravel(), u[hy, :].ravel(),
            u[lo, lo].ravel(), u[lo, hx].ravel(), u[hy, lo].ravel(), u[hy, hx].ravel()]


def _act_download(csim, st, c, cur):
    assert c.same(st.download(), cur)
    return cur


def _act_download_interior(csim, st, c, cur):
    assert np.array_equal(st.download_interior(), cur[1:-1, 1:-1])
    return cur


def _act_checksum(csim, st, c, cur):
    assert st.checksum() == csim.checksum_host(cur[1:-1, 1:-1])
    return cur


def _act_minmax(csim, st, c, cur):
    mn, mx = st.minmax()   # whole array, ghosts included; the four corners are nobody's: the stepper's own
    corners = st.download()[[0, 0, -1, -1], [0, -1, 0, -1]]
    vals = np.concatenate([cur[c.mask], corners])
    assert mn == vals.min() and mx == vals.max()
    return cur


def _act_sum(csim, st, c, cur):
    s = st.sum()
    inner = cur[1:-1, 1:-1]
    assert abs(s - float(np.sum(inner))) <= 1e-9 * np.abs(inner).sum()   # tolerance of test_reductions
    return cur


def _act_snapshot(csim, st, c, cur):
    st.snapshot_begin()
    run(st, 3)                    # the time loop goes on while the copy is in flight
    snap = st.snapshot_wait()
    assert np.array_equal(snap, cur[1:-1, 1:-1])
    return c.advance(cur, 3)


def _act_upload(csim, st, c, cur):
    other = c.field(1)
    st.upload(other)
    assert np.array_equal(st.download(), other)   # the write wins over the run it follows, corners included
    return other


def _act_init_gaussian(csim, st, c, cur):
    args = (1.0, 0.1, 0.3, 0.6)
    st.init_gaussian(*args)
    got = st.download()
    fresh = csim.Stepper(self_neighbor_decomp(csim, c.nx, c.ny, c.sides), 1.0, 1.0, c.codes)   # never ran anything
    fresh.init_gaussian(*args)
    assert np.array_equal(got, fresh.download())
    fresh.close()
    host = ora.gaussian_global(c.nx, c.ny, A=args[0], sigma_frac=args[1], xc_frac=args[2], yc_frac=args[3])
    assert np.abs(got - host).max() <= 4 * np.finfo(float).eps   # exp() may differ by an ulp (test_gpu_parity.py)
    return got


def _act_exchange_halos(csim, st, c, cur):
    st.exchange_halos()
    assert c.same(st.download(), _wrapped(c, cur))   # physical sides untouched
    return cur                                       # (every step wraps the linked ghosts anew)


def _act_tune(csim, st, c, cur):
    st.tune(D, DT, VX, VY)
    return cur


def _act_keep_warm(csim, st, c, cur):
    st.keep_warm(D, DT, VX, VY, 0.003)
    return cur


def _option(key, value):
    def act(csim, st, c, cur):
        if key == "overlap":
            set_overlap(csim, st, value)
        else:
            st.set_option(key, value)
            assert st.get_option(key) == value
        return cur
    return act


def _act_halo_pack(csim, st, c, cur):
    st.set_option("external_halo", 1)
    lines = st.halo_pack()
    edges = [cur[1:-1, 1], cur[1:-1, -2], cur[1, 1:-1], cur[-2, 1:-1]]
    for k in range(4):
        assert (lines[k] is None) == (not c.sides[k])
        if c.sides[k]:
            assert np.array_equal(lines[k], edges[k]), k
    st.set_option("external_halo", 0)
    return cur


def _act_faces_pack(csim, st, c, cur):
    depth = min(3, c.smallest)
    st.set_option("external_halo", 1)
    faces = st.faces_pack(depth)
    peers, _ = st.faces_neighbors(depth)
    assert sum(p >= 0 for p in peers) == (8 if all(c.sides) else 2)
    for d, want in enumerate(_faces(cur, depth)):
        assert (faces[d] is None) == (peers[d] < 0)
        if faces[d] is not None:
            assert np.array_equal(faces[d], want), d
    st.set_option("external_halo", 0)
    return cur


def _act_run(csim, st, c, cur):
    return cur   # the run() every case ends with is the call under test


ENTRY_POINTS = {
    "download": _act_download, "download_interior": _act_download_interior, "checksum": _act_checksum,
    "minmax": _act_minmax, "sum": _act_sum, "snapshot": _act_snapshot, "upload": _act_upload,
    "init_gaussian": _act_init_gaussian, "exchange_halos": _act_exchange_halos, "tune": _act_tune,
    "keep_warm": _act_keep_warm, "relay_0": _option("relay", 0), "relay_events_1": _option("relay_events", 1),
    "overlap_0": _option("overlap", 0), "overlap_1": _option("overlap", 1), "overlap_3": _option("overlap", 3),
    "overlap_4": _option("overlap", 4), "fuse_3": _option("fuse", 3), "fuse_0": _option("fuse", 0),
    "halo_pack": _act_halo_pack, "faces_pack": _act_faces_pack, "run": _act_run,
}
DEFAULTS = (("overlap", 5), ("relay", 1), ("relay_events", 0), ("fuse", -1), ("external_halo", 0))


@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_entry_point_directly_after_a_relay_run(csim, geom, entry):
    """a stepper left by run() with 1, 2 and 3 relay passes (the state on s_relay[1], [0], [1]); the entry point is
    the very next API call.  Readers return the oracle's state after the run, writers win over the run, and 9 more
    steps from there (two passes, or 2 + 2 + .. + 1 on the two-row tile) equal the oracle again — a stale tail or a
    lost hand-over shows as a wrong field."""
    c = case(csim, geom)
    st = c.stepper(csim)
    for passes in (1, 2, 3):
        for k, v in DEFAULTS:
            st.set_option(k, v)
        st.upload(c.field())
        n = steps_for(csim, passes, -1, c.smallest)
        assert all(t >= 2 for t in csim.pass_schedule(n, c.smallest, -1))
        run(st, n)
        after = ENTRY_POINTS[entry](csim, st, c, c.want(n))
        run(st, 9)
        got = st.download()
        want = c.want(n + 9) if after is c.want(n) else c.advance(after, 9)
        assert c.same(got, want), (passes, n, int((got != want)[c.mask].sum()))
    st.close()


# ---- c. schedules changed on one live stepper ------------------------------------------------------------------
SCHEDULES = {"0": (0, 1), "1": (1, 1), "3": (3, 1), "4": (4, 1), "5": (5, 1), "5_relay0": (5, 0)}


def _every_ordered_pair(names):
    """a closed walk through the complete digraph on `names` (loops included) that takes every edge once
    (Hierholzer): consecutive entries cover every ordered pair of schedules"""
    out_edges = {a: list(names) for a in names}
    stack, walk = [names[0]], []
    while stack:
        a = stack[-1]
        if out_edges[a]:
            stack.append(out_edges[a].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


@pytest.mark.parametrize("check", ["every_segment", "at_the_end"])
@pytest.mark.parametrize("geom", ["torus_1160x300", "leftright_1160x300_ddnp", "torus_128x2"])
def test_schedules_changed_on_one_live_stepper(csim, geom, check):
    """one stepper, one uploaded field, 37 seeded segments (options, then run(k), k = 1..20) whose schedules cover
    every ordered pair of {0, 1, 3, 4, 5, 5 without the relay}, keep_warm and timer reads in between: the full array
    equals the oracle's after every segment ("at_the_end": the same sequence without the downloads, whose settle
    and wait would otherwise stand between every two schedules)."""
    c = case(csim, geom)
    walk = _every_ordered_pair(list(SCHEDULES))
    assert len(walk) == 37 and set(zip(walk, walk[1:])) == {(a, b) for a in SCHEDULES for b in SCHEDULES}
    rng = np.random.default_rng(20240)
    st = c.stepper(csim)
    st.set_option("profile", 1)
    st.upload(c.field())
    total = 0
    for seg, name in enumerate(walk):
        overlap, relay = SCHEDULES[name]
        set_overlap(csim, st, overlap)
        opts = dict(relay=relay, relay_events=int(rng.integers(0, 2)), fuse=int(rng.choice([-1, -1, 0, 2, 3, 5, 6, 7])),
                    direct_faces=int(rng.integers(0, 2)), rows_per_chunk=int(rng.choice([0, 0, 3, 20])))
        k = int(rng.integers(1, 21))
        for key, v in opts.items():
            if rng.random() < 0.7 or key == "relay":
                st.set_option(key, v)
        run(st, k)
        total += k
        if seg % 5 == 2:
            st.keep_warm(D, DT, VX, VY, 0.002)
        if seg % 4 == 1:
            ms, launches, covered = st.kernel_time()
            assert covered == total and math.isfinite(ms) and ms > 0   # profile = 1: every pass since the upload
            st.comm_time()
        if check == "every_segment":
            got = st.download()
            assert c.same(got, c.want(total)), (seg, name, opts, k, total)
    got = st.download()
    assert c.same(got, c.want(total)), total
    st.close()


# ---- d. what the timers count ----------------------------------------------------------------------------------
def chains(calls, overlap):
    """passes of the given run() calls (one depth list per call) whose exchange chain ran on the comm stream inside a
    PROF_COMM bracket, by the schedules' definitions (include/csim.h, "overlap"; passes.cpp):
      0      the exchange is serial on the compute stream: none;
      1, 3   a fused pass hides the NEXT pass's exchange under its bulk: one chain per fused pass that has a fused
             successor in the SAME call (the first pass of a call pays its exchange unhidden on the compute stream,
             and a single-step pass posts its edge lines without a bracket), so cutting a run into two calls takes
             one chain away;
      4, 5   a fused pass hides its OWN exchange: one chain per fused pass, however the run is cut."""
    if overlap == 0:
        return 0
    if overlap in (1, 3):
        return sum(sum(1 for a, b in zip(d, d[1:]) if a >= 2 and b >= 2) for d in calls)
    return sum(sum(1 for t in d if t >= 2) for d in calls)


def read_timers(st):
    """kernel_time of every kind and comm_time, with nothing in front of them: {kind: (ms, launches)}, (ms, passes)"""
    kt = {T: st.kernel_time(T) for T in range(1, 8)}
    return kt, st.comm_time()


def check_times(kt, ct):
    for ms, n in list(kt.values()) + [ct]:
        assert math.isfinite(ms) and (ms > 0 if n > 0 else ms == 0), (kt, ct)


def assert_timers_zero(st):
    kt, ct = read_timers(st)
    assert all(v == (0.0, 0) for v in kt.values()) and ct == (0.0, 0), (kt, ct)


@pytest.mark.parametrize("overlap,relay", [(0, 1), (1, 1), (3, 1), (4, 1), (4, 0), (5, 1), (5, 0)])
@pytest.mark.parametrize("geom", ["torus_1160x300", "leftright_1160x300_ddnp", "torus_128x2"])
def test_timers_straight_after_run_count_the_planners_passes(csim, geom, overlap, relay):
    """profile = 1 on the torus: the timers are read as the very next call after run() — no sync, no download —,
    whichever of them comes first; a multi-rank pass is ONE bracket around its sweep launch(es) (frame and bulk of a
    split pass are not counted separately), so launches of kind T == the planner's passes of depth T."""
    c = case(csim, geom)
    st = c.stepper(csim)
    if not set_overlap(csim, st, overlap):
        st.close()
        return
    st.set_option("relay", relay)
    st.set_option("profile", 1)
    for first in ("comm_time", "reset_timers"):   # (kernel_time comes first everywhere below)
        st.upload(c.field())
        run(st, 20)
        if first == "comm_time":
            assert st.comm_time()[1] == chains([csim.pass_schedule(20, c.smallest, -1)], overlap)
        st.reset_timers()
        assert_timers_zero(st)
    for fuse in (-1, 0, 2, 5, 7):
        st.set_option("fuse", fuse)
        for steps in (20, 9, 1):
            depths = csim.pass_schedule(steps, c.smallest, fuse)
            assert sum(depths) == steps
            st.upload(c.field())
            run(st, steps)
            kt, ct = read_timers(st)
            assert {T: kt[T][1] for T in kt} == {T: depths.count(T) for T in kt}, (fuse, steps, depths, kt)
            assert sum(T * kt[T][1] for T in kt) == steps
            assert ct[1] == chains([depths], overlap), (fuse, steps, depths, ct)
            check_times(kt, ct)
            got = st.download()
            assert c.same(got, c.want(steps)), (fuse, steps)
            st.reset_timers()
            assert_timers_zero(st)
            if len(depths) < 2:
                continue
            # the same passes in two run() calls
            a = sum(depths[:len(depths) // 2])
            da, db = csim.pass_schedule(a, c.smallest, fuse), csim.pass_schedule(steps - a, c.smallest, fuse)
            st.upload(c.field())
            run(st, a)
            run(st, steps - a)
            kt, ct2 = read_timers(st)
            assert {T: kt[T][1] for T in kt} == {T: (da + db).count(T) for T in kt}, (fuse, steps, da, db, kt)
            assert ct2[1] == chains([da, db], overlap), (fuse, steps, da, db, ct2)
            if da + db == depths and overlap in (0, 4, 5):
                assert ct2[1] == ct[1]
            check_times(kt, ct2)
            assert c.same(st.download(), c.want(steps)), (fuse, steps, a)
            st.reset_timers()
    st.close()


@pytest.mark.parametrize("overlap", [5, 1, 0])
def test_sampled_profile_counts_every_third_pass_and_profile_0_nothing(csim, overlap):
    """profile = 3: passes 0, 3, 6, .. counted from the option's setting are bracketed, across run() calls;
    profile = 0: nothing is."""
    c = case(csim, "leftright_1160x300_ddnp")
    st = c.stepper(csim)
    set_overlap(csim, st, overlap)
    st.upload(c.field())
    run(st, 6)                      # unprofiled passes in front must not count
    st.set_option("profile", 3)     # restarts the pass counter
    calls = [csim.pass_schedule(n, c.smallest, -1) for n in (20, 9, 14, 2, 1, 16)]
    for n in (20, 9, 14, 2, 1, 16):
        run(st, n)
    every = [t for d in calls for t in d]
    sampled = every[::3]
    kt, ct = read_timers(st)
    assert sum(n for _, n in kt.values()) == math.ceil(len(every) / 3)
    assert {T: kt[T][1] for T in kt} == {T: sampled.count(T) for T in kt}, (every, kt)
    check_times(kt, ct)
    total = 6 + sum(every)
    assert c.same(st.download(), c.want(total))
    st.set_option("profile", 0)
    st.reset_timers()
    run(st, 20)
    assert_timers_zero(st)
    assert c.same(st.download(), c.want(total + 20))
    st.close()


def _single_rank_field(nx, ny, seed):
    """random interior, a random value on each ghost line (Periodic ghosts must survive), as the single-rank fuzz of
    tests/test_gpu_parity.py"""
    rng = np.random.default_rng(seed)
    u0 = np.zeros((ny + 2, nx + 2))
    u0[1:-1, 1:-1] = rng.standard_normal((ny, nx))
    u0[0, :], u0[-1, :], u0[:, 0], u0[:, -1] = rng.standard_normal(4)
    return u0


def test_single_rank_brackets_count_every_launch_once(csim):
    """one rank, profile = 1: ONE event pair per run of equal launches.  run() calls whose depth patterns alternate (so
    brackets open and close), timer reads between some of them: no launch lost, none counted twice."""
    nx, ny, bc = 384, 200, csim.bc_codes("dnpd")
    u0 = _single_rank_field(nx, ny, 5)
    st = csim.Stepper.single(nx, ny, 1.0, 1.0, bc)
    st.set_option("profile", 1)
    st.upload(u0)
    want = u0.copy()
    expect = {T: 0 for T in range(1, 8)}
    for call, (steps, fuse) in enumerate([(8, -1), (3, -1), (8, 7), (1, -1), (5, 2), (12, -1), (2, 7), (7, 7), (7, 3),
                                          (1, 0), (4, 0), (20, -1), (9, 2), (13, 7)]):
        st.set_option("fuse", fuse)
        depths = csim.pass_schedule(steps, min(nx, ny), fuse, tile_cells=nx * ny)
        assert sum(depths) == steps
        for t in depths:
            expect[t] += 1
        run(st, steps)
        if call % 3 == 1:   # a read between two run() calls
            kt = {T: st.kernel_time(T) for T in expect}
            assert {T: kt[T][1] for T in kt} == expect, (call, kt)
            check_times(kt, (0.0, 0))
    kt, ct = read_timers(st)
    assert {T: kt[T][1] for T in kt} == expect and ct == (0.0, 0), (kt, ct)
    assert len([T for T in expect if expect[T]]) >= 5
    check_times(kt, ct)
    got = st.download()
    ora.run_single(want, 1.0, 1.0, D, VX, VY, DT, bc, sum(T * n for T, n in expect.items()))
    assert np.array_equal(got, want)
    st.reset_timers()
    assert_timers_zero(st)
    # sampled form on one rank
    st.set_option("profile", 3)
    st.set_option("fuse", -1)
    calls = [csim.pass_schedule(n, min(nx, ny), -1, tile_cells=nx * ny) for n in (20, 9, 14, 2)]
    for n in (20, 9, 14, 2):
        run(st, n)
    every = [t for d in calls for t in d]
    kt, _ = read_timers(st)
    assert {T: kt[T][1] for T in kt} == {T: every[::3].count(T) for T in kt}, (every, kt)
    ora.run_single(want, 1.0, 1.0, D, VX, VY, DT, bc, sum(every))
    assert np.array_equal(st.download(), want)
    st.close()


# ---- e. the event pool ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(), dict(relay=0), dict(overlap=1)], ids=["default", "relay_0", "overlap_1"])
@pytest.mark.parametrize("sides,bc", [((1, 1, 1, 1), "dddd"), ((1, 1, 0, 0), "ddnp")])
def test_one_run_past_the_event_pool(csim, sides, bc, opts):
    """profile = 1 uses 4 events per multi-rank pass, the pool holds 2048: ONE run() of 550 passes folds the pool in
    the middle of the run, with passes in flight on whichever streams the schedule uses.  The run succeeds, the field
    is the oracle's, every pass is counted."""
    nx, ny, steps = 64, 32, 1100
    rng = np.random.default_rng(77)
    u0 = rng.standard_normal((ny + 2, nx + 2))
    codes = csim.bc_codes(bc)
    st = csim.Stepper(self_neighbor_decomp(csim, nx, ny, sides), 1.0, 1.0, codes)
    st.comm_init(csim.comm_unique_id())
    for k, v in opts.items():
        st.set_option(k, v)
    st.set_option("fuse", 2)
    st.set_option("profile", 1)
    depths = csim.pass_schedule(steps, min(nx, ny), 2)
    assert depths == [2] * 550
    st.upload(u0)
    run(st, steps)
    kt, ct = read_timers(st)
    assert {T: kt[T][1] for T in kt} == {T: depths.count(T) for T in kt}, kt
    assert ct[1] == chains([depths], st.get_option("overlap"))
    check_times(kt, ct)
    got = st.download()
    st.close()
    want = torus_oracle(u0, 1.0, 1.0, D, VX, VY, DT, steps, sides, codes)
    m = CORNERLESS(ny, nx)
    assert np.array_equal(got[m], want[m]), int((got != want)[m].sum())


def test_many_short_single_rank_runs_past_the_event_pool(csim):
    """one rank: 1100 run() calls of alternating depth open 1100 brackets (2200 events) with no timer read in between,
    then one read: the counts add up and the field is the oracle's."""
    nx, ny, bc = 64, 32, csim.bc_codes("dnpd")
    u0 = _single_rank_field(nx, ny, 78)
    st = csim.Stepper.single(nx, ny, 1.0, 1.0, bc)
    st.set_option("profile", 1)
    st.upload(u0)
    expect = {T: 0 for T in range(1, 8)}
    for call in range(1100):
        n = 2 + call % 2
        for t in csim.pass_schedule(n, min(nx, ny), -1, tile_cells=nx * ny):
            expect[t] += 1
        run(st, n)
    assert expect[2] == 550 and expect[3] == 550
    kt, ct = read_timers(st)
    assert {T: kt[T][1] for T in kt} == expect, kt
    check_times(kt, ct)
    got = st.download()
    st.close()
    want = u0.copy()
    ora.run_single(want, 1.0, 1.0, D, VX, VY, DT, bc, 550 * 5)
    assert np.array_equal(got, want)
