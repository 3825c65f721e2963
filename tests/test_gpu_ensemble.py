"""The batched stepper (csim_ensemble_*): B members of one grid shape, each with its own field and (D, dt, vx, vy),
must each come out exactly as the reference run alone with its own parameters — compared BIT for bit (integer views:
+0 and -0 differ; NaN cells by position) with oracle.cpu_oracle.run_single, whole arrays, ghost ring included."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cpu_oracle as ora
from test_gpu_diffusion_only import nasty_field, same_bits

pytestmark = pytest.mark.gpu

# (D, dt, vx, vy): both signs of each component, a zero component of either axis, both zero, D = 0, -0 as a
# velocity, several dt
PHYS12 = [
    (0.05, 0.1, 0.5, 0.25), (0.05, 0.1, -0.5, 0.25), (0.05, 0.1, 0.5, -0.25), (0.05, 0.1, -0.5, -0.25),
    (0.05, 0.05, 0.0, 0.3), (0.05, 0.05, 0.4, 0.0), (0.1, 0.05, 0.0, 0.0), (0.0, 0.1, 0.5, 0.25),
    (0.0, 0.2, -0.3, 0.0), (0.02, 0.2, 0.0, -0.4), (0.05, 0.1, -0.0, 0.25), (0.1, 0.02, 0.3, 0.3),
]


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def random_fields(B, nx, ny, seed):
    """random interiors AND ghost rings (a periodic side keeps its stored ghosts, the others are overwritten)"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, ny + 2, nx + 2))


def oracle_runs(u0s, phys, bc, steps, dx=1.0, dy=1.0, value=0.0):
    ora.lib()  # loaded (built if need be) once, before the threads use it

    def one(k):
        u = u0s[k].copy()
        D, dt, vx, vy = phys[k]
        ora.run_single(u, dx, dy, D, vx, vy, dt, bc, steps, value=value)
        return u
    with ThreadPoolExecutor(8) as ex:  # the oracle's C loop releases the GIL
        return list(ex.map(one, range(len(u0s))))


def run_ensemble(csim, u0s, phys, bc, steps, dx=1.0, dy=1.0, fuse=None, calls=None, bc_value=0.0):
    B, ny2, nx2 = u0s.shape
    e = csim.Ensemble(B, nx2 - 2, ny2 - 2, dx, dy, bc, bc_value)
    if fuse is not None:
        e.set_option("fuse", fuse)
    e.upload_all(u0s)
    e.set_physics(*[[p[k] for p in phys] for k in range(4)])
    for n in (calls or [steps]):
        e.run(n)
    e.sync()
    return e


def assert_members(got, want, what):
    bad = [k for k in range(len(want)) if not same_bits(got[k], want[k])]
    assert not bad, f"{what}: members {bad} differ from the oracle"


@pytest.mark.parametrize("bcs", ["dddd", "nnnn", "dnpd"])
@pytest.mark.parametrize("steps", [1, 4, 7, 20, 23])
def test_mixed_physics_130x67(csim, bcs, steps):
    bc = csim.bc_codes(bcs)
    u0s = random_fields(12, 130, 67, seed=steps)
    want = oracle_runs(u0s, PHYS12, bc, steps)
    e = run_ensemble(csim, u0s, PHYS12, bc, steps)
    assert_members(e.download_all(), want, f"{bcs} {steps} steps")
    # the same run in single steps only, and split over two calls: the same bits
    if steps in (7, 23):
        assert_members(run_ensemble(csim, u0s, PHYS12, bc, steps, fuse=0).download_all(), want, "fuse=0")
        assert_members(run_ensemble(csim, u0s, PHYS12, bc, steps, calls=[5, steps - 5]).download_all(), want, "5 + rest")


@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (5, 1), (3, 140), (130, 3)])
@pytest.mark.parametrize("bcs", ["dnpd", "nnnn"])
def test_tiny_and_thin(csim, shape, bcs):
    nx, ny = shape
    bc = csim.bc_codes(bcs)
    phys = PHYS12[:3]
    u0s = random_fields(3, nx, ny, seed=nx * 1000 + ny)
    want = oracle_runs(u0s, phys, bc, 9)
    e = run_ensemble(csim, u0s, phys, bc, 9)
    assert_members(e.download_all(), want, f"{nx}x{ny}")
    if min(nx, ny) < 4:
        assert e.get_option("depth_used") == 1


def test_isolation_of_a_nasty_member(csim):
    nx, ny, steps = 700, 160, 9
    bc = csim.bc_codes("dnpd")
    phys = [(0.05, 0.1, 0.5, -0.25), (0.1, 0.1, 0.0, 0.0), (0.02, 0.05, -0.3, 0.0)]
    clean = random_fields(3, nx, ny, seed=5)
    with_nasty = clean.copy()
    with_nasty[1] = nasty_field(nx, ny, 3)
    got_clean = run_ensemble(csim, clean, phys, bc, steps).download_all()
    got_nasty = run_ensemble(csim, with_nasty, phys, bc, steps).download_all()
    for k in (0, 2):
        assert same_bits(got_nasty[k], got_clean[k]), f"member {k} depends on its neighbour"
    assert_members(got_nasty, oracle_runs(with_nasty, phys, bc, steps), "with a nasty member")


def test_one_member_equals_stepper(csim):
    nx, ny, steps = 384, 200, 9
    D, dt, vx, vy = 0.05, 0.1, 0.5, -0.25
    bc = csim.bc_codes("dnpd")
    u0 = random_fields(1, nx, ny, seed=11)
    st = csim.Stepper.single(nx, ny, 1.0, 1.0, bc)
    st.upload(u0[0])
    st.run(D, dt, vx, vy, steps)
    e = run_ensemble(csim, u0, [(D, dt, vx, vy)], bc, steps)
    assert e.checksums() == [st.checksum()]
    assert same_bits(e.download(0), st.download())
    st.close()


def test_64_members_512(csim):
    B, n, steps = 64, 512, 20
    bc = csim.bc_codes("dddd")
    rng = np.random.default_rng(64)
    phys = [(0.05 * rng.random(), 0.05 + 0.1 * rng.random(), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5))
            for _ in range(B)]
    phys[3] = (0.05, 0.1, 0.0, 0.0)
    u0s = random_fields(B, n, n, seed=65)
    want = oracle_runs(u0s, phys, bc, steps)
    e = run_ensemble(csim, u0s, phys, bc, steps)
    assert e.checksums() == [csim.checksum_host(w[1:-1, 1:-1]) for w in want]
    for k in (0, 3, 31, 63):
        assert same_bits(e.download(k), want[k]), f"member {k}"


def test_diagnostics(csim):
    nx, ny, B = 130, 67, 5
    bc = csim.bc_codes("dnpd")
    u0s = random_fields(B, nx, ny, seed=7)
    e = run_ensemble(csim, u0s, PHYS12[:B], bc, 6)
    arrs = e.download_all()
    assert e.checksums() == [csim.checksum_host(a[1:-1, 1:-1]) for a in arrs]
    mm = e.minmax()
    assert np.array_equal(mm[:, 0], arrs.min(axis=(1, 2))) and np.array_equal(mm[:, 1], arrs.max(axis=(1, 2)))
    # the sum adds per-block partials in a fixed order: the same field gives the same bits every time, and it agrees
    # with numpy's (pairwise) sum to rounding
    s = e.sums()
    assert np.array_equal(s, e.sums())
    np.testing.assert_allclose(s, arrs[:, 1:-1, 1:-1].sum(axis=(1, 2)), rtol=1e-12, atol=1e-12 * nx * ny)


def test_gaussian_member(csim):
    e = csim.Ensemble(2, 64, 48)
    e.init_gaussian(1, A=2.0, sigma_frac=0.1, xc_frac=0.3, yc_frac=0.6)
    st = csim.Stepper.single(64, 48)
    st.init_gaussian(A=2.0, sigma_frac=0.1, xc_frac=0.3, yc_frac=0.6)
    assert same_bits(e.download(1), st.download())
    assert not e.download(0).any()
    st.close()


@pytest.mark.parametrize("bcs", ["dnpd", "pppp"])
def test_gaussian_over_an_uploaded_member_equals_stepper(csim, bcs):
    """init_gaussian replaces the member's whole array, ghost ring included (a periodic side keeps that ring for good),
    and later steps match a Stepper that saw the same calls"""
    nx, ny = 130, 67
    D, dt, vx, vy = 0.05, 0.1, 0.5, -0.25
    bc = csim.bc_codes(bcs)
    u0s = random_fields(3, nx, ny, seed=21)
    e = run_ensemble(csim, u0s, [(D, dt, vx, vy)] * 3, bc, 5)
    e.init_gaussian(1, A=2.0, sigma_frac=0.1, xc_frac=0.3, yc_frac=0.6)
    st = csim.Stepper.single(nx, ny, 1.0, 1.0, bc)
    st.upload(u0s[1])
    st.run(D, dt, vx, vy, 5)
    st.init_gaussian(A=2.0, sigma_frac=0.1, xc_frac=0.3, yc_frac=0.6)
    assert same_bits(e.download(1), st.download())
    e.run(9)
    st.run(D, dt, vx, vy, 9)
    assert same_bits(e.download(1), st.download())
    assert e.checksums()[1] == st.checksum()
    st.close()


def test_depth_used_of_short_runs(csim):
    T = csim.ensemble_plan(0, 64, 64)[0]
    e = run_ensemble(csim, random_fields(2, 64, 64, seed=3), PHYS12[:2], [0, 0, 0, 0], T - 1)
    assert e.get_option("depth_used") == 1  # fewer steps than one pass: single steps only
    e.run(T)
    assert e.get_option("depth_used") == T


def test_argument_errors(csim):
    E = csim.CsimError
    for args in [(0, 8, 8), (2, 0, 8), (2, 8, 0)]:
        with pytest.raises(E) as ex:
            csim.Ensemble(*args)
        assert ex.value.code == 1
    h = csim.C.c_void_p()
    assert csim.lib().csim_ensemble_create(2, 8, 8, 2, 1.0, 1.0, csim._i4((0, 0, 0, 0)), 0.0, csim.C.byref(h)) == 1
    e = csim.Ensemble(2, 8, 8)
    u = np.ones((10, 10))
    for bad in [lambda: e.upload(2, u), lambda: e.upload(-1, u), lambda: e.download(2),
                lambda: e.init_gaussian(5), lambda: e.set_physics(0.1, np.nan, 0.0, 0.0),
                lambda: e.set_physics(0.1, [0.1, np.inf], 0.0, 0.0),
                lambda: e.set_option("nope", 1), lambda: e.set_option("fuse", 5),
                lambda: e.set_option("depth_used", 1), lambda: e.get_option("nope")]:
        with pytest.raises(E) as ex:
            bad()
        assert ex.value.code == 1
    for bad in [lambda: e.set_option("contract", 1), lambda: e.get_option("contract")]:
        with pytest.raises(E) as ex:
            bad()
        assert ex.value.code == 5
    with pytest.raises(E) as ex:
        e.run(1)  # no physics yet
    assert ex.value.code == 4
    # still usable
    e.upload(1, u)
    e.set_physics(0.1, 0.1, 0.0, 0.0)
    e.run(5)
    want = u.copy()
    ora.run_single(want, 1.0, 1.0, 0.1, 0.0, 0.0, 0.1, [0, 0, 0, 0], 5)
    assert same_bits(e.download(1), want)
    assert e.get_option("depth_used") == csim.ensemble_plan(5, 8, 8)[0] > 1 and e.get_option("fuse") == -1 and e.get_option("fused_2c") == 1
