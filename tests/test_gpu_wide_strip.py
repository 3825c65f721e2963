"""Wide strips (stepper option "wide_strips": the interior between the bands is cut into strips of four columns per
lane, sweepO_march with NC = 4 in csrc/sweep_core.hpp, planned by csrc/sweep_plan.cpp) against the oracle, bit for bit.
"wide_strips" = 1 takes a wide strip wherever one fits.  The shapes are the smallest that exercise each seam of the
plan, derived from the strip geometry of the depth under test (at seven steps per pass: 359, 360, 608, 849, 1100
columns); the three wide bodies are reached through the verdict word, as tests/test_gpu_screen_lease.py reaches the
narrow ones: a positive field (leased 12-operation body), one negative cell (leased 14-operation body), patches of
1e300 and NaN (no lease: the reference's own sequence)."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cpu_oracle as ora

pytestmark = pytest.mark.gpu

D, DT = 0.05, 0.1
LEASE = 128
BASE = dict(pow2_v=1, lease_acquire_after=0, lease_steps=LEASE, wide_strips=1)
SIGNS = [(0.5, 0.25), (0.5, -0.25), (-0.5, 0.25)]      # sign pairs (1,1), (1,0), (0,1): the flavours with a wide kernel
SPACINGS = [(1.0, 1.0), (0.5, 0.25)]                   # DIV 0, DIV 1
BCS = ["dddd", "nnnn", "dnpd"]
CELL = (15, 200)    # row, column of the cell a refused field differs in: inside the first wide strip of every shape


def geometry(T):
    """(narrow stride, wide stride, overlap) of strips at T steps per pass: strip_stride, strip_overlap of sweep_plan.hpp"""
    tp = 2 * ((T + 1) // 2)
    return 128 - 2 * tp, 256 - 2 * tp, tp


def shapes(T):
    """name -> (nx, ny, rows_per_chunk): no wide strip fits; exactly one; one and narrow strips on the right; odd nx (the
    right ghost column is the second of its pair); several, a 28-column remainder, chunks of 6 rows and of a ragged height"""
    s2, s4, tp = geometry(T)
    one = s2 + tp + s4
    return {"none": (one - 1, 30, 0), "one": (one, 30, 0), "one_and_right": (one + 248, 40, 0),
            "odd": (s2 + 3 * s4 + 17, 37, 0), "several_6": (s2 + 4 * s4 + 28, 64, 6), "several_ragged": (s2 + 4 * s4 + 28, 64, 11)}


def wide_fits(nx, ny, T):
    s2, s4, tp = geometry(T)
    hb = T - 1 + (6 - (3 * (T - 1)) % 6) % 6   # whole_groups(T, T - 1): the height of a band
    return T in (6, 7) and nx >= s2 + tp + s4 and ny >= 2 * hb + 6


assert [shapes(7)[k][0] for k in ("none", "one", "one_and_right", "odd", "several_6")] == [359, 360, 608, 849, 1100]


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    assert pkg.device_name().startswith("gfx950"), pkg.device_name()
    return pkg


def hotspot(nx, ny, background=1e-3):
    j, i = np.mgrid[0:ny + 2, 0:nx + 2]
    u = background + np.exp(-((i - 0.4 * nx) ** 2 + (j - 0.55 * ny) ** 2) / (2.0 * (0.08 * nx) ** 2))
    u[0, :] = u[-1, :] = u[:, 0] = u[:, -1] = 0.0
    return u


def field(kind, nx, ny):
    """kind -> (u0, the verdict word a Dirichlet ring leaves)"""
    u0 = hotspot(nx, ny)
    if kind == "negative":
        u0[CELL] = -0.5
        return u0, 1
    if kind == "unleased":
        u0[CELL[0]:CELL[0] + 2, CELL[1]:CELL[1] + 3] = 1e300
        u0[CELL[0] + 3, CELL[1] + 40:CELL[1] + 42] = np.nan
        return u0, 0
    return u0, 3


_want = {}


def oracle(key, u0, dx, dy, vx, vy, dt, steps, bc):
    key = (key, dx, dy, vx, vy, dt, steps, bc)
    if key not in _want:
        w = u0.copy()
        with np.errstate(all="ignore"):
            ora.run_single(w, dx, dy, D, vx, vy, dt, ora.bc_codes(bc), steps, 0.0)
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


def gpu(csim, u0, dx, dy, vx, vy, dt, calls, opts, bc):
    ny, nx = u0.shape[0] - 2, u0.shape[1] - 2
    st = csim.Stepper.single(nx, ny, dx, dy, csim.bc_codes(bc), 0.0)
    for k, v in {**BASE, **opts}.items():
        st.set_option(k, v)
    st.upload(u0)
    for n in calls:
        st.run(D, dt, vx, vy, n)
    word, active = st.get_option("lease_word"), st.get_option("wide_strips_active")
    got = st.download()
    st.close()
    return got, word, active


def assert_bits(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, int((np.isnan(got) != np.isnan(want)).sum()))
    ok = ~np.isnan(want)
    bad = got[ok].view(np.int64) != want[ok].view(np.int64)
    assert not bad.any(), (what, int(bad.sum()))


@pytest.mark.parametrize("body", ["leased_p2", "negative", "unleased"])
@pytest.mark.parametrize("shape", list(shapes(7)))
@pytest.mark.parametrize("fuse", [6, 7, -1])
def test_wide_strips_match_the_oracle(csim, fuse, shape, body):
    """every seam of the plan x depth x body, and inside: DIV 0 / 1 x three sign pairs x three boundary mixes; the whole
    array is compared, so the ghost ring after the final pass is too"""
    T = fuse if fuse > 0 else 7
    nx, ny, rpc = shapes(T)[shape]
    u0, word_want = field(body, nx, ny)
    for dx, dy in SPACINGS:
        for vx, vy in SIGNS:
            dt = min(DT, csim.safe_dt(dx, dy, vx, vy, D))
            steps = 2 * T   # a fixed depth is balanced over the passes of a call: two passes of exactly T
            for bc in BCS:
                want = oracle((body, nx, ny), u0, dx, dy, vx, vy, dt, 1 + steps, bc)
                got, word, active = gpu(csim, u0, dx, dy, vx, vy, dt, [1, steps], dict(fuse=fuse, rows_per_chunk=rpc), bc)
                what = (shape, nx, ny, fuse, body, dx, vx, vy, bc)
                if fuse > 0:   # (the automatic plan of so small a field prefers depths without a wide kernel)
                    assert active == int(wide_fits(nx, ny, T)), what
                if bc == "dddd":
                    assert word == word_want, what
                assert_bits(got, want, what)


@pytest.mark.parametrize("fuse", [6, 7])
@pytest.mark.parametrize("bc", BCS)
def test_wide_and_narrow_on_one_stepper(csim, fuse, bc):
    """"wide_strips" 0 and 1 on the same stepper and inputs: identical fields and identical ghost rings after a final pass"""
    nx, ny, rpc = shapes(fuse)["several_ragged"]
    u0 = hotspot(nx, ny)
    st = csim.Stepper.single(nx, ny, 1.0, 1.0, csim.bc_codes(bc), 0.0)
    for k, v in {**BASE, "fuse": fuse, "rows_per_chunk": rpc}.items():
        st.set_option(k, v)
    got = {}
    for wide in (0, 1, 0):
        st.set_option("wide_strips", wide)
        st.upload(u0)
        st.run(D, DT, 0.5, 0.25, 1)
        st.run(D, DT, 0.5, 0.25, 3 * fuse)
        assert st.get_option("wide_strips_active") == wide
        got.setdefault(wide, []).append(st.download())
    st.close()
    want = oracle(("hot", nx, ny), u0, 1.0, 1.0, 0.5, 0.25, DT, 3 * fuse + 1, bc)
    for wide, fields in got.items():
        for g in fields:
            assert_bits(g, want, (wide, fuse, bc))


def test_where_wide_strips_are_not_taken(csim):
    """the option is an offer: both velocities negative, general velocities, the lease switched off and depths without a
    wide kernel keep the narrow plan — and stay bit-identical"""
    nx, ny, _ = shapes(7)["several_6"]
    u0 = hotspot(nx, ny)
    for vx, vy, opts in [(-0.5, -0.25, dict(fuse=7)), (0.3, 0.2, dict(fuse=7)), (0.5, 0.25, dict(fuse=7, screen_lease=0)),
                         (0.5, 0.25, dict(fuse=5)), (0.5, 0.25, dict(fuse=7, wide_strips=0)), (0.5, 0.25, dict(fuse=7, pow2_v=0))]:
        want = oracle(("hot", nx, ny), u0, 1.0, 1.0, vx, vy, DT, 14, "dddd")
        got, _, active = gpu(csim, u0, 1.0, 1.0, vx, vy, DT, [14], opts, "dddd")
        assert active == 0, (vx, vy, opts)
        assert_bits(got, want, (vx, vy, opts))
    # the default (2) takes wide strips only on tiles where they were measured to pay: never on one this small
    got, _, active = gpu(csim, u0, 1.0, 1.0, 0.5, 0.25, DT, [14], dict(fuse=7, wide_strips=2), "dddd")
    assert active == 0
    assert_bits(got, oracle(("hot", nx, ny), u0, 1.0, 1.0, 0.5, 0.25, DT, 14, "dddd"), "default")
