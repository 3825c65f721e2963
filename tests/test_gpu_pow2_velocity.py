"""The 12-operation interior body for power-of-two velocities (stepper option "pow2_v", M_FAST_P2 in
csrc/sweep_core.hpp) against the oracle, bit for bit: on a field with many interior-body tiles (3+ strips, short chunks,
as test_fused_2c_guard_values_near_overflow uses) that carries patches on both sides of the screen's lower bound L
(about 2^-600 = 2.4e-181 for these parameters), down to the smallest subnormal, exact zeros, -0.0, and patches on both
sides of its upper bound; with the form on and off; where the host must leave it off; and on the path bench.py times."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cpu_oracle as ora

pytestmark = pytest.mark.gpu

NX, NY = 700, 160
VELOCITIES = [(0.5, 0.25), (0.5, -0.25), (-0.5, 0.25), (-0.5, -0.25), (1.0, 0.125), (2.0, 0.5)]
SPACINGS = [(1.0, 1.0), (0.5, 0.25)]   # DIV 0, DIV 1
D, DT = 0.05, 0.1


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    assert pkg.device_name().startswith("gfx950"), pkg.device_name()
    return pkg


@pytest.fixture(scope="module")
def field():
    """Interior tiles of this shape at depths 4..7: strips 1..5 of 7 (columns ~110..560), chunks of 18 rows between the
    bottom and top bands.  Every patch lies well inside them; a tile that loads one below L (or -0.0 on the flavour that
    screens it, or one above the upper bound) must fall back to the reference's sequence, the others run the new body."""
    rng = np.random.default_rng(2024)
    u = np.zeros((NY + 2, NX + 2))
    u[1:-1, 1:-1] = rng.standard_normal((NY, NX))
    u[24:30, 130:150] *= 1e-150     # above L: stays on the 12-operation body
    u[24:30, 250:270] *= 1e-250     # below L from here on
    u[24:30, 370:390] *= 1e-290
    u[24:30, 490:510] *= 1e-305
    u[60:66, 130:150] *= 1e-310     # subnormal
    u[60:66, 250:270] = 5e-324 * np.sign(u[60:66, 250:270])
    u[60:66, 370:390] = 0.0
    u[62, 372:380] = 1.0            # ... with a few cells standing in the zeros
    u[60:66, 490:510] = -0.0
    u[63, 495] = 0.5
    u[96:102, 130:150] *= 1e300     # below the upper bound of the new body's screen (3.5e303 .. 1.7e306 in these cases)
    u[113:119, 130:150] *= 1e305    # around it
    u[96:102, 250:270] *= 4e306     # above it, around fast_thr (1.3e307 here): plain body, some cells overflow
    u[96:102, 370:390] *= 1e-200    # just below L
    u[96:102, 490:510] *= 1e-170    # just above L
    u[130:136, 200:260][::2, ::3] = 0.0
    u[130:136, 400:460][::2, ::3] = -0.0
    return u


_want = {}


def oracle(field, dx, dy, vx, vy, dt, steps):
    key = (dx, dy, vx, vy, dt, steps)
    if key not in _want:
        w = field.copy()
        with np.errstate(all="ignore"):
            ora.run_single(w, dx, dy, D, vx, vy, dt, ora.bc_codes("dddd"), steps)
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


def gpu(csim, u0, dx, dy, Dv, vx, vy, dt, steps, opts, bc="dddd", calls=None):
    ny, nx = u0.shape[0] - 2, u0.shape[1] - 2
    st = csim.Stepper.single(nx, ny, dx, dy, csim.bc_codes(bc))
    for k, v in opts.items():
        st.set_option(k, v)
    st.upload(u0)
    for n in calls or [steps]:
        st.run(Dv, dt, vx, vy, n)
    active = st.get_option("pow2_v_active")
    got = st.download()
    st.close()
    return got, active


def assert_bits(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, int((np.isnan(got) != np.isnan(want)).sum()))
    ok = ~np.isnan(want)
    bad = got[ok].view(np.int64) != want[ok].view(np.int64)
    assert not bad.any(), (what, int(bad.sum()))


@pytest.mark.parametrize("dx,dy", SPACINGS)
@pytest.mark.parametrize("vx,vy", VELOCITIES)
@pytest.mark.parametrize("fuse", [4, 5, 6, 7])
def test_parity_with_patches_around_the_screen(csim, field, dx, dy, vx, vy, fuse):
    steps = fuse + 3
    dt = min(DT, csim.safe_dt(dx, dy, vx, vy, D))
    L, hi = csim.pow2_velocity_screen(D, dt, vx, vy, dx, dy)[:2]
    assert 1e-195 < L < 1e-172 and 1e302 < hi < 4e306, (L, hi)   # the patches straddle both bounds
    want = oracle(field, dx, dy, vx, vy, dt, steps)
    assert np.isfinite(want).sum() > 0.9 * want.size
    for on in (1, 0):
        got, active = gpu(csim, field, dx, dy, D, vx, vy, dt, steps, dict(fuse=fuse, rows_per_chunk=18, pow2_v=on))
        assert active == on
        assert_bits(got, want, (on, fuse))


@pytest.mark.parametrize("what,vx,vy,Dv,dt,opts", [
    ("not a power of two", 0.3, 0.25, D, DT, {}),
    ("not a power of two (y)", 0.5, 0.3, D, DT, {}),
    ("zero component", 0.5, 0.0, D, DT, {}),
    ("zero component (x)", 0.0, 0.25, D, DT, {}),
    ("fused_2c off", 0.5, 0.25, D, DT, dict(fused_2c=0)),
    ("wildly unstable", 0.5, 0.25, 3.0e18, 1.0, {}),
])
def test_inactive_cases_are_unchanged(csim, field, what, vx, vy, Dv, dt, opts):
    u0 = field if Dv == D else np.where(np.abs(field) > 1e300, 1.0, field)
    want = u0.copy()
    with np.errstate(all="ignore"):
        ora.run_single(want, 1.0, 1.0, Dv, vx, vy, dt, ora.bc_codes("dddd"), 9)
    for on in (1, 0):
        got, active = gpu(csim, u0, 1.0, 1.0, Dv, vx, vy, dt, 9, dict(fuse=6, rows_per_chunk=18, pow2_v=on, **opts))
        assert active == 0, what
        assert_bits(got, want, (what, on))


def test_contract_keeps_its_own_form(csim, field):
    """option "contract" is the coefficient form (not bit-identical to the reference): pow2_v must not touch it"""
    u0 = np.where(np.abs(field) > 1e300, 1.0, field)
    runs = [gpu(csim, u0, 1.0, 1.0, D, 0.5, 0.25, DT, 9, dict(fuse=6, rows_per_chunk=18, contract=1, pow2_v=on)) for on in (1, 0)]
    assert runs[0][1] == 0 and runs[1][1] == 0
    assert np.array_equal(runs[0][0].view(np.int64), runs[1][0].view(np.int64))


def test_bench_path_on_a_small_hotspot(csim):
    """what bench.py's preflight does on 16384^2 — the hotspot, then 1 + 7 + 32 steps with automatic depths — at
    1024 x 512 against the oracle, with the form on (the path bench.py times) and off"""
    nx, ny = 1024, 512
    vx, vy = 0.5, 0.25
    dt = min(DT, csim.safe_dt(1.0, 1.0, vx, vy, D))
    y, x = np.mgrid[0:ny, 0:nx]
    r2 = ((x + 0.5) - 0.5 * nx) ** 2 + ((y + 0.5) - 0.5 * ny) ** 2
    u0 = np.zeros((ny + 2, nx + 2))
    u0[1:-1, 1:-1] = np.exp(-r2 / (2.0 * (0.05 * nx) ** 2))
    assert u0[1:-1, 1:-1].min() > csim.pow2_velocity_screen(D, dt, vx, vy)[0]   # every interior tile passes the screen
    want = u0.copy()
    ora.run_single(want, 1.0, 1.0, D, vx, vy, dt, ora.bc_codes("dddd"), 40)
    for on in (1, 0):
        got, active = gpu(csim, u0, 1.0, 1.0, D, vx, vy, dt, 40, dict(pow2_v=on), calls=[1, 7, 32])
        assert active == on
        assert_bits(got, want, on)


def test_default_takes_the_form_on_large_tiles_only(csim):
    """pow2_v = 2 (default): on from 6e7 cells (where it was measured to pay), off below; 1 forces it on, as every test above does"""
    st = csim.Stepper.single(NX, NY, 1.0, 1.0, csim.bc_codes("dddd"))
    assert st.get_option("pow2_v") == 2
    st.init_gaussian()
    st.run(D, DT, 0.5, 0.25, 4)
    assert st.get_option("pow2_v_active") == 0
    st.set_option("pow2_v", 1)
    st.run(D, DT, 0.5, 0.25, 4)
    assert st.get_option("pow2_v_active") == 1
    with pytest.raises(csim.CsimError):
        st.set_option("pow2_v", 3)
    st.close()
    big = csim.Stepper.single(8192, 7400, 1.0, 1.0, csim.bc_codes("dddd"))   # 6.06e7 cells
    big.init_gaussian()
    big.run(D, DT, 0.5, 0.25, 4)
    assert big.get_option("pow2_v_active") == 1
    big.run(D, DT, 0.3, 0.25, 4)
    assert big.get_option("pow2_v_active") == 0
    big.close()
