"""The screen lease (stepper option "screen_lease": one reduction judges the whole field, interior tiles then march
without their screen — M_LEASED / M_LEASED_P2 in csrc/sweep_core.hpp) against the oracle, bit for bit, on the smallest
shapes that have interior tiles at seven steps per pass (five strips, chunks of 18 rows between the bands): leases that
must be granted, fields that must be refused one reason at a time, and the bookkeeping of a lease's life (renewals,
uploads, parameter changes, a renewal that is refused).  "pow2_v" = 1 takes the 12-operation body at this size and
"lease_acquire_after" = 0 spends the first reduction in front of the first pass; leases of 128 steps, so that the
power-of-two spacing (a0 = 0.6, a lower bound that sinks 0.74 binades per step) still admits an ordinary field."""
import math

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cpu_oracle as ora

pytestmark = pytest.mark.gpu

D, DT = 0.05, 0.1
SHAPES = [(512, 256), (460, 200)]
LEASE = 128
BASE = dict(pow2_v=1, lease_acquire_after=0, lease_steps=LEASE, rows_per_chunk=18)
CELL = (100, 250)   # row, column of the one cell a refused field differs in: inside an interior tile at every depth


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    assert pkg.device_name().startswith("gfx950"), pkg.device_name()
    return pkg


def hotspot(nx, ny, background=1e-3, sigma=None):
    """a positive field: a hotspot on a background, the ring zero"""
    j, i = np.mgrid[0:ny + 2, 0:nx + 2]
    sigma = sigma or 0.08 * nx
    u = background + np.exp(-((i - 0.4 * nx) ** 2 + (j - 0.55 * ny) ** 2) / (2.0 * sigma ** 2))
    u[0, :] = u[-1, :] = u[:, 0] = u[:, -1] = 0.0
    return u


_want = {}


def oracle(key, u0, dx, dy, vx, vy, dt, steps, bc="dddd", value=0.0):
    key = (key, dx, dy, vx, vy, dt, steps, bc, value)
    if key not in _want:
        w = u0.copy()
        with np.errstate(all="ignore"):
            ora.run_single(w, dx, dy, D, vx, vy, dt, ora.bc_codes(bc), steps, value)
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


def gpu(csim, u0, dx, dy, vx, vy, dt, calls, opts, bc="dddd", value=0.0):
    ny, nx = u0.shape[0] - 2, u0.shape[1] - 2
    st = csim.Stepper.single(nx, ny, dx, dy, csim.bc_codes(bc), value)
    for k, v in {**BASE, **opts}.items():
        st.set_option(k, v)
    st.upload(u0)
    for n in calls:
        st.run(D, dt, vx, vy, n)
    word, reductions = st.get_option("lease_word"), st.get_option("lease_reductions")
    got = st.download()
    st.close()
    return got, word, reductions


def assert_bits(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, int((np.isnan(got) != np.isnan(want)).sum()))
    ok = ~np.isnan(want)
    bad = got[ok].view(np.int64) != want[ok].view(np.int64)
    assert not bad.any(), (what, int(bad.sum()))


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("dx,dy", [(1.0, 1.0), (0.5, 0.25)])
@pytest.mark.parametrize("vx,vy", [(0.5, 0.25), (0.5, -0.25), (-0.5, 0.25)])
@pytest.mark.parametrize("fuse", [4, 5, 6, 7, -1])
def test_granted_lease_is_bit_identical(csim, nx, ny, dx, dy, vx, vy, fuse):
    u0 = hotspot(nx, ny)
    dt = min(DT, csim.safe_dt(dx, dy, vx, vy, D))
    steps = 2 * max(fuse, 4) + 3
    M_req, m_req = csim.screen_lease_bounds(D, dt, vx, vy, dx, dy, LEASE)[:2]
    assert 0 < m_req < 1e-100 and M_req > 1e100
    want = oracle(("hot", nx, ny), u0, dx, dy, vx, vy, dt, steps)
    on, word, red = gpu(csim, u0, dx, dy, vx, vy, dt, [steps], dict(fuse=fuse))
    assert (word, red) == (3, 1)
    off, word0, red0 = gpu(csim, u0, dx, dy, vx, vy, dt, [steps], dict(fuse=fuse, screen_lease=0))
    assert (word0, red0) == (0, 0)
    assert_bits(on, want, "lease on")
    assert_bits(off, want, "lease off")


@pytest.mark.parametrize("vx,vy,word_want", [(0.3, 0.2, 1), (-0.3, 0.25, 1), (-0.5, -0.25, 3)])
def test_flavours_without_a_leased_p2_body(csim, vx, vy, word_want):
    """general velocities lease the upper bound only (bit 0, M_LEASED); both velocities negative keeps the screened
    12-operation body whatever the word says"""
    nx, ny = SHAPES[1]
    u0 = hotspot(nx, ny)
    want = oracle(("hot", nx, ny), u0, 1.0, 1.0, vx, vy, DT, 17)
    for lease in (1, 0):
        got, word, _ = gpu(csim, u0, 1.0, 1.0, vx, vy, DT, [17], dict(fuse=7, screen_lease=lease))
        assert word == (word_want if lease else 0)
        assert_bits(got, want, lease)


REFUSED = [("negative cell", -0.5, 1), ("interior zero", 0.0, 1), ("minus zero", -0.0, 1), ("1e-250", 1e-250, 1),
           ("1e300", 1e300, 0), ("inf", np.inf, 0), ("nan", np.nan, 0)]


@pytest.mark.parametrize("what,v,word_want", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_refused_lease_one_cell(csim, nx, ny, what, v, word_want):
    M_req, m_req = csim.screen_lease_bounds(D, DT, 0.5, 0.25, 1.0, 1.0, LEASE)[:2]
    assert 1e-250 < m_req < 1e-100 and 1e100 < M_req < 1e300
    u0 = hotspot(nx, ny)
    u0[CELL] = v
    for fuse in (7, 4):
        want = oracle((what, nx, ny), u0, 1.0, 1.0, 0.5, 0.25, DT, 2 * fuse + 3)
        got, word, red = gpu(csim, u0, 1.0, 1.0, 0.5, 0.25, DT, [2 * fuse + 3], dict(fuse=fuse))
        assert (word, red) == (word_want, 1), what
        assert_bits(got, want, (what, fuse))   # NaN: the same cells, every other cell bit for bit


@pytest.mark.parametrize("what,bc,value", [("negative Dirichlet value", "dddd", -1.0), ("negative Periodic ghost", "dpdp", 0.0),
                                          ("minus zero Periodic ghost", "pddd", 0.0)])
def test_refused_lease_ring(csim, what, bc, value):
    nx, ny = SHAPES[0]
    u0 = hotspot(nx, ny)
    if "Periodic" in what:   # a stored ghost of a Periodic side is never rewritten
        neg = -0.25 if "negative" in what else -0.0
        if bc[3] == "p":
            u0[-1, 200:210] = neg
        if bc[0] == "p":
            u0[120:130, 0] = neg
    want = oracle((what, nx, ny), u0, 1.0, 1.0, 0.5, 0.25, DT, 17, bc, value)
    got, word, red = gpu(csim, u0, 1.0, 1.0, 0.5, 0.25, DT, [17], dict(fuse=7), bc, value)
    assert (word, red) == (1, 1), what
    assert_bits(got, want, what)


def reductions_by_the_rule(calls, R, depth):
    """lease_for_pass with lease_acquire_after = 0 and passes of `depth` steps (calls of one step are single-step passes)"""
    held, age, count = False, 0, 0
    for n in calls:
        for t in ([1] if n == 1 else [depth] * (n // depth)):
            if t == depth and (not held or age + t > R):
                held, age, count = True, 0, count + 1
            age += t
    return count


def test_lifecycle_renewals(csim):
    nx, ny = SHAPES[1]
    u0 = hotspot(nx, ny)
    calls = [8, 1, 4, 1, 1, 1, 4, 12, 4, 20, 16, 8, 20]
    assert sum(calls) == 100 and all(n == 1 or n % 4 == 0 for n in calls)
    st = csim.Stepper.single(nx, ny, 1.0, 1.0, csim.bc_codes("dddd"))
    for k, v in {**BASE, "fuse": 4, "lease_steps": 16}.items():
        st.set_option(k, v)
    st.upload(u0)
    want = u0.copy()
    for k, n in enumerate(calls):
        st.run(D, DT, 0.5, 0.25, n)
        ora.run_single(want, 1.0, 1.0, D, 0.5, 0.25, DT, ora.bc_codes("dddd"), n)
        assert st.get_option("lease_reductions") == reductions_by_the_rule(calls[:k + 1], 16, 4), (k, n)
        assert st.get_option("lease_word") == 3
        assert_bits(st.download(), want, (k, n))
    assert st.get_option("lease_reductions") >= 6
    st.close()


def test_upload_and_physics_change(csim):
    nx, ny = SHAPES[0]
    u0 = hotspot(nx, ny)
    bad = u0.copy()
    bad[CELL] = 0.0
    bc = ora.bc_codes("dddd")
    st = csim.Stepper.single(nx, ny, 1.0, 1.0, csim.bc_codes("dddd"))
    for k, v in {**BASE, "fuse": 7}.items():
        st.set_option(k, v)
    st.upload(u0)
    st.run(D, DT, 0.5, 0.25, 14)
    assert (st.get_option("lease_word"), st.get_option("lease_reductions")) == (3, 1)
    # a refusing field after a grant: the word is cleared before any pass can read it
    st.upload(bad)
    assert st.get_option("lease_word") == 0
    st.run(D, DT, 0.5, 0.25, 14)
    assert (st.get_option("lease_word"), st.get_option("lease_reductions")) == (1, 2)
    want = bad.copy()
    ora.run_single(want, 1.0, 1.0, D, 0.5, 0.25, DT, bc, 14)
    assert_bits(st.download(), want, "after the upload")
    # other parameters: judged anew, against the new bounds
    st.upload(u0)
    st.run(D, DT, 0.5, 0.25, 7)
    assert (st.get_option("lease_word"), st.get_option("lease_reductions")) == (3, 3)
    st.run(D, 0.05, 0.5, 0.25, 7)
    assert (st.get_option("lease_word"), st.get_option("lease_reductions")) == (3, 4)
    st.set_option("pow2_v", 0)       # what the field is judged against changes: judged anew
    st.run(D, 0.05, 0.5, 0.25, 7)
    assert (st.get_option("lease_word"), st.get_option("lease_reductions")) == (1, 5)
    want = u0.copy()
    ora.run_single(want, 1.0, 1.0, D, 0.5, 0.25, DT, bc, 7)
    ora.run_single(want, 1.0, 1.0, D, 0.5, 0.25, 0.05, bc, 14)
    assert_bits(st.download(), want, "after the parameter changes")
    st.set_option("screen_lease", 0)
    assert st.get_option("lease_word") == 0
    st.close()


def test_a_renewal_is_refused_when_the_minimum_sinks(csim):
    """Dirichlet(0) inflow: the corner cell next to two ring zeros, far from the narrow hotspot, shrinks by about 0.915
    per step (a0 + 2 x 0.005 from its equally small neighbours).  A background of twice m_req is admitted, and sixteen
    steps on — some 2^-1.9 lower — the renewal must refuse bit 1."""
    nx, ny = SHAPES[1]
    M_req, m_req, eta, a0 = csim.screen_lease_bounds(D, DT, 0.5, 0.25, 1.0, 1.0, 16)
    L = csim.pow2_velocity_screen(D, DT, 0.5, 0.25)[0]
    assert 2 * L < m_req < 2.0 ** -560
    u0 = hotspot(nx, ny, background=2.0 * m_req, sigma=7.0)
    assert u0[1, 1] == 2.0 * m_req and math.log2(a0 * (1 - eta)) * 16 < -1.0   # the bound allows for a sink below m_req
    st = csim.Stepper.single(nx, ny, 1.0, 1.0, csim.bc_codes("dddd"))
    for k, v in {**BASE, "fuse": 4, "lease_steps": 16}.items():
        st.set_option(k, v)
    st.upload(u0)
    want = u0.copy()
    words = []
    for n in (8, 8, 4, 12, 16):
        st.run(D, DT, 0.5, 0.25, n)
        ora.run_single(want, 1.0, 1.0, D, 0.5, 0.25, DT, ora.bc_codes("dddd"), n)
        words.append(st.get_option("lease_word"))
        assert_bits(st.download(), want, (n, words))
    assert words[0] == 3 and words[1] == 3, words      # granted, and held through its sixteen steps
    assert 1 in words[2:], words                       # a renewal refused the 12-operation lease, not the upper bound
    assert st.get_option("lease_reductions") == 3
    assert want[1, 1] < m_req
    st.close()


def test_external_halo_stepper_has_no_lease(csim):
    nx, ny = SHAPES[1]
    u0 = hotspot(nx, ny)
    want = oracle(("hot", nx, ny), u0, 1.0, 1.0, 0.5, 0.25, DT, 17)
    got, word, red = gpu(csim, u0, 1.0, 1.0, 0.5, 0.25, DT, [17], dict(fuse=7, external_halo=1))
    assert (word, red) == (0, 0)
    assert_bits(got, want, "external")
