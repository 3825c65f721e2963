"""Host-only logic of the batched stepper (no GPU): the pass plan of csim_ensemble_run and the grouping of members
into one launch per upwind-sign class."""
import pytest

from __graft_entry__ import load_package


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


def test_plan_splits_into_fused_passes_and_single_steps(csim):
    T = csim.ensemble_plan(0, 512, 512)[0]
    assert 2 <= T <= 7
    for n in range(0, 40):
        depth, q, r = csim.ensemble_plan(n, 512, 512)
        assert (depth, q, r) == (T, n // T, n % T)
        assert q * depth + r == n


def test_plan_depth_capped_by_the_grid(csim):
    T = csim.ensemble_plan(0, 512, 512)[0]
    for nx, ny in [(1, 1), (2, 5), (5, 1), (3, 140), (130, 3), (T - 1, 512), (512, T - 1)]:
        assert csim.ensemble_plan(23, nx, ny) == (1, 0, 23), (nx, ny)
    assert csim.ensemble_plan(23, T, T)[0] == T


def test_plan_fuse_option(csim):
    for fuse in (0, 1):
        assert csim.ensemble_plan(23, 512, 512, fuse) == (1, 0, 23)
    for bad in (-2, 2, 7):
        with pytest.raises(csim.CsimError) as ex:
            csim.ensemble_plan(23, 512, 512, bad)
        assert ex.value.code == 1
    with pytest.raises(csim.CsimError):
        csim.ensemble_plan(-1, 512, 512)


def test_sign_classes(csim):
    c = csim.ensemble_sign_class
    assert c(0.05, 0.1, 0.5, 0.25) == 4      # both >= 0
    assert c(0.05, 0.1, -0.5, 0.25) == 1
    assert c(0.05, 0.1, 0.5, -0.25) == 3
    assert c(0.05, 0.1, -0.5, -0.25) == 0
    assert c(0.05, 0.1, 0.0, 0.0) == 8       # diffusion only (screened)
    assert c(0.05, 0.1, -0.0, 0.25) == 7     # -0 is a zero component
    assert c(0.05, 0.1, 0.0, -0.25) == 6
    assert c(0.05, 0.1, 0.5, 0.0) == 5
    assert c(0.05, 0.1, -0.5, 0.0) == 2
    # without the screen (fused_2c off) or with IEEE division, a zero component is "v >= 0"
    assert c(0.05, 0.1, 0.0, 0.0, fused_2c=0) == 4
    assert c(0.05, 0.1, 0.0, -0.25, dx=0.3, dy=0.3) == 3


def test_one_launch_per_class_present(csim):
    n = csim.ensemble_launches
    assert n([4] * 64) == 1
    assert n([4, 4, 1, 8, 1, 4]) == 3
    assert n(list(range(9)) * 3) == 9
    with pytest.raises(csim.CsimError):
        n([9])
