"""Per-cell ensemble statistics (csim_ensemble_stats*): mean and variance must equal np.mean / np.var over the member
axis of download_all() BIT for bit (integer views, NaN cells by position), min and max np.fmin.reduce /
np.fmax.reduce by value, whole arrays, ghost ring included."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from test_gpu_diffusion_only import same_bits
from test_gpu_ensemble import PHYS12, random_fields

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


def numpy_stats(a, ddof):
    with np.errstate(all="ignore"):
        return (np.mean(a, axis=0), np.var(a, axis=0, ddof=ddof), np.fmin.reduce(a, axis=0),
                np.fmax.reduce(a, axis=0))


def assert_stats(got, a, ddof, what):
    mean, var, lo, hi = numpy_stats(a, ddof)
    assert got.mean.shape == mean.shape, what
    assert same_bits(got.mean, mean), f"{what}: mean (ddof {ddof})"
    assert same_bits(got.var, var), f"{what}: var (ddof {ddof})"
    np.testing.assert_array_equal(got.min, lo, err_msg=f"{what}: min")
    np.testing.assert_array_equal(got.max, hi, err_msg=f"{what}: max")


def ensemble_with(csim, u0s, bc=(0, 0, 0, 0)):
    B, ny2, nx2 = u0s.shape
    e = csim.Ensemble(B, nx2 - 2, ny2 - 2, 1.0, 1.0, bc)
    e.upload_all(u0s)
    return e


@pytest.mark.parametrize("bcs", ["dddd", "nnnn", "dnpd"])
@pytest.mark.parametrize("steps", [0, 1, 4, 7, 23])
def test_after_runs_130x67(csim, bcs, steps):
    u0s = random_fields(12, 130, 67, seed=100 + steps)
    e = ensemble_with(csim, u0s, csim.bc_codes(bcs))
    if steps:  # steps == 0: uploaded fields, no set_physics
        e.set_physics(*[[p[k] for p in PHYS12] for k in range(4)])
        e.run(steps)
    a = e.download_all()
    for ddof in (0, 1):
        assert_stats(e.stats(ddof), a, ddof, f"{bcs} {steps} steps")


@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (130, 67), (512, 512)])
@pytest.mark.parametrize("B", [1, 2, 3, 12, 64])
def test_shapes_and_members(csim, shape, B):
    nx, ny = shape
    e = ensemble_with(csim, random_fields(B, nx, ny, seed=B * 7 + nx))
    a = e.download_all()
    for ddof in ((0,) if B == 1 else (0, 1)):
        assert_stats(e.stats(ddof), a, ddof, f"{B} x {nx}x{ny}")


def test_members_loaded_by_four_waves(csim):
    B = 200  # above the one-wave form's limit, within LDS
    u0s = nasty_members(B, 48, 40, seed=200)
    e = ensemble_with(csim, u0s)
    a = e.download_all()
    for ddof in (0, 1):
        assert_stats(e.stats(ddof), a, ddof, "200 x 48x40")


def test_more_members_than_lds_holds(csim):
    B = 700  # past the 320 members the kernel keeps in LDS: the rest are read again
    u0s = nasty_members(B, 48, 40, seed=700)
    e = ensemble_with(csim, u0s)
    a = e.download_all()
    for ddof in (0, 1):
        assert_stats(e.stats(ddof), a, ddof, "700 x 48x40")


def test_larger_than_the_infinity_cache(csim):
    B, n = 64, 1024  # 64 x 1026^2 doubles = 539 MB
    u0s = np.random.default_rng(1024).random((B, n + 2, n + 2))
    e = ensemble_with(csim, u0s)
    del u0s
    got = e.stats(1)
    assert_stats(got, e.download_all(), 1, "64 x 1024^2")


def nasty_members(B, nx, ny, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((B, ny + 2, nx + 2))
    pick = lambda n: tuple(rng.integers(0, [B, ny + 2, nx + 2], size=(n, 3)).T)  # noqa: E731
    for v, n in [(np.nan, 40), (np.inf, 30), (-np.inf, 30), (0.0, 40), (-0.0, 40), (5e-324, 20), (-5e-324, 20),
                 (2.2e-308, 20), (1e308, 40), (-1e308, 40)]:
        a[pick(n)] = v
    a[:, 2, 3] = -0.0        # every member -0: numpy's mean is +0
    a[:, 4, 4] = np.nan      # every member NaN
    a[:, 5, 6] = 1e308       # the sum overflows
    a[:, 6, 1] = 5e-324      # subnormal mean and variance
    a[0, 7, 2], a[-1, 7, 2] = np.inf, -np.inf
    a[:-1, 8, 3], a[-1, 8, 3] = np.nan, 0.5  # one finite member among NaNs
    return a


@pytest.mark.parametrize("B", [2, 5, 12])
def test_special_values(csim, B):
    e = ensemble_with(csim, nasty_members(B, 37, 23, seed=B))
    a = e.download_all()
    assert np.signbit(a[:, 2, 3]).all()
    for ddof in (0, 1):
        got = e.stats(ddof)
        assert_stats(got, a, ddof, f"special values, B = {B}")
    assert got.mean[2, 3] == 0.0 and not np.signbit(got.mean[2, 3])
    assert np.isnan(got.min[4, 4]) and np.isnan(got.max[4, 4]) and got.min[8, 3] == a[-1, 8, 3]


@pytest.mark.parametrize("B", [15, 16, 17, 31, 32, 33, 79, 80, 81, 127, 128, 129, 319, 320, 321])
def test_member_count_seams(csim, B):
    """either side of the kernel's member-count edges: a batch of 16 members and two of them, the switch to four
    loading waves (80 / 81), four cooperative batches (128) and the LDS limit (320 / 321)"""
    e = ensemble_with(csim, nasty_members(B, 37, 23, seed=1000 + B))
    a = e.download_all()
    for ddof in (0, 1):
        assert_stats(e.stats(ddof), a, ddof, f"member-count seam, B = {B}")


def test_null_outputs_are_skipped(csim):
    u0s = random_fields(3, 20, 10, seed=3)
    e = ensemble_with(csim, u0s)
    var = np.full((12, 22), 7.0)
    lib, C = csim.lib(), csim.C
    assert lib.csim_ensemble_stats(e._h, 0, None, var.ctypes.data_as(C.POINTER(C.c_double)), None, None) == 0
    assert same_bits(var, np.var(u0s, axis=0))
    assert lib.csim_ensemble_stats(e._h, 0, None, None, None, None) == 0


def test_async_captures_the_state_before_the_run(csim):
    bc = csim.bc_codes("dnpd")
    u0s = random_fields(12, 130, 67, seed=42)
    phys = [[p[k] for p in PHYS12] for k in range(4)]
    e, plain = ensemble_with(csim, u0s, bc), ensemble_with(csim, u0s, bc)
    e.set_physics(*phys)
    plain.set_physics(*phys)
    for k in (7, 20, 1):
        before = e.download_all()
        e.stats_begin(1)
        e.run(k)
        got = e.stats_wait()
        assert_stats(got, before, 1, f"begin; run({k}); wait")
        plain.run(k)
        assert same_bits(e.download_all(), plain.download_all()), f"run({k}) changed by the statistics"
    # two _begin in a row: the second one's state is returned
    e.stats_begin(0)
    e.run(4)
    e.stats_begin(0)
    now = e.download_all()
    assert_stats(e.stats_wait(), now, 0, "second begin")
    # a synchronous call between _begin and _wait leaves the captured result alone
    e.stats_begin(1)
    e.run(3)
    e.stats(0)
    assert_stats(e.stats_wait(), now, 1, "begin; run; stats; wait")
    with pytest.raises(csim.CsimError) as ex:
        e.stats_wait()  # nothing in flight any more
    assert ex.value.code == 4


def test_errors(csim):
    E = csim.CsimError
    fresh = csim.Ensemble(2, 8, 8)
    with pytest.raises(E) as ex:
        fresh.stats_wait()  # never begun
    assert ex.value.code == 4
    one = csim.Ensemble(1, 8, 8)
    for bad in [lambda: fresh.stats(2), lambda: fresh.stats(-1), lambda: fresh.stats_begin(2),
                lambda: one.stats(1), lambda: one.stats_begin(1)]:
        with pytest.raises(E) as ex:
            bad()
        assert ex.value.code == 1
    lib, C = csim.lib(), csim.C
    p = C.POINTER(C.c_double)()
    assert lib.csim_ensemble_stats(None, 0, None, None, None, None) == 1
    assert lib.csim_ensemble_stats_begin(None, 0) == 1
    assert lib.csim_ensemble_stats_wait(None, C.byref(p), None, None, None) == 1
    # still usable after the refusals
    assert_stats(one.stats(0), one.download_all(), 0, "after errors")
