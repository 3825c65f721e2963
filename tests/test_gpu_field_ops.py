"""The operators at the reference's own granularity (csim_diffusion_step, csim_advection_step, csim_fused_step on
Fields, csim_apply_boundary, csim_field_fill / _copy / _swap: k_unit_op, k_ring_copy, k_ghost_fill, k_fill) against
the oracle's restatement of the reference (oracle/cpu_oracle.py, itself pinned to the reference by
tests/test_oracle_golden.py), bit for bit, at the shapes where their 256-thread blocks and their max(nx, ny)-sized
launches have seams: 255 / 256 / 257 and 511 / 513 columns, one row, one column, ny >> nx, and with subnormals, 1e300,
signed zeros, +Inf and NaN in the data.  NaN masks must agree; every other cell is compared through its bits."""
import itertools

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cpu_oracle as ora

pytestmark = pytest.mark.gpu

SHAPES = [(255, 2), (256, 1), (257, 70), (511, 3), (513, 3), (1, 300), (300, 1), (700, 3), (3, 700), (1, 1)]
SPACINGS = [(1.0, 1.0), (0.5, 0.25), (0.7, 1.3)]  # no division, reciprocal powers of two, IEEE division
VELOCITIES = [(0.5, -0.25), (-0.3, 0.2), (0.0, 0.4), (-0.6, 0.0)]  # both signs of both, one zero component each
D, DT = 0.07, 0.1
SENTINEL = -777.25
CASES = [(nx, ny, dx, dy) for (nx, ny) in SHAPES for (dx, dy) in SPACINGS]
CASE_IDS = [f"{nx}x{ny}-dx{dx}-dy{dy}" for nx, ny, dx, dy in CASES]

BC_SHAPES = [(257, 3), (3, 257), (1, 1), (300, 260)]
BC_MIXES = ["".join(m) for m in itertools.product("dnp", repeat=4)]
MASK_MIXES = ["dnpd", "nnnn", "dddd", "pnnp"]
BC_VALUES = [1.5, -0.0]


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    assert pkg.device_name().startswith("gfx950"), pkg.device_name()
    return pkg


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def same_cells(got, want):
    """NaN in the same cells, every other cell the same bits"""
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan) and
            np.array_equal(got.view(np.int64)[~nan], want.view(np.int64)[~nan]))


def noise(nx, ny, seed):
    """Gaussian noise; the four ghost lines are non-zero and differ from each other and from the interior"""
    rng = np.random.default_rng([seed, nx, ny])
    u = rng.standard_normal((ny + 2, nx + 2))
    u[0, :] += 10.0
    u[-1, :] -= 20.0
    u[:, 0] += 30.0
    u[:, -1] -= 40.0
    return u


def planted(nx, ny, seed):
    """noise with blocks of subnormals, 1e300, +0 / -0, +Inf and NaN (3 columns x 2 rows each, clipped)"""
    u = noise(nx, ny, seed)
    blocks = [((0.10, 0.15), [5e-324, -2.5e-310, 1e-308]), ((0.35, 0.60), [1e300, -1e300, 1e300]),
              ((0.50, 0.30), [0.0, -0.0, 0.0]), ((0.70, 0.80), [np.inf] * 3), ((0.90, 0.45), [np.nan] * 3)]
    for (fj, fi), vals in blocks:
        j, i = int(fj * (ny + 2)), int(fi * (nx + 2))
        for dj in range(2):
            for di in range(3):
                if j + dj < ny + 2 and i + di < nx + 2:
                    u[j + dj, i + di] = vals[di]
    return u


def fields(nx, ny):
    return [("noise", noise(nx, ny, 1)), ("planted", planted(nx, ny, 2))]


def ring(a):
    return np.concatenate([a[0, :], a[-1, :], a[:, 0], a[:, -1]])


@pytest.mark.parametrize("nx,ny,dx,dy", CASES, ids=CASE_IDS)
def test_diffusion_step(csim, nx, ny, dx, dy):
    fu, fo = csim.Field(nx, ny, 1, dx, dy), csim.Field(nx, ny, 1, dx, dy)
    for name, u in fields(nx, ny):
        fu.upload(u)
        fo.fill(SENTINEL)
        csim.diffusion_step(fu, fo, D, DT)
        got = fo.download()
        want = np.full_like(u, SENTINEL)
        with np.errstate(all="ignore"):
            ora.diffusion_step(u, want, dx, dy, D, DT)
        assert same_cells(got, want), name
        assert same_bits(ring(got), ring(u)), name  # the ring copy, corners included
        assert not (got[1:-1, 1:-1] == SENTINEL).any(), name
        assert same_bits(fu.download(), u), name


@pytest.mark.parametrize("nx,ny,dx,dy", CASES, ids=CASE_IDS)
def test_advection_step_accumulates(csim, nx, ny, dx, dy):
    fu, fo = csim.Field(nx, ny, 1, dx, dy), csim.Field(nx, ny, 1, dx, dy)
    o = noise(nx, ny, 3) * 0.5 + 2.0
    for (name, u), (vx, vy) in itertools.product(fields(nx, ny), VELOCITIES):
        fu.upload(u)
        fo.upload(o)
        csim.advection_step(fu, fo, vx, vy, DT)
        got = fo.download()
        want = o.copy()
        ora.advection_step(u, want, dx, dy, vx, vy, DT)
        assert same_cells(got, want), (name, vx, vy)
        assert same_bits(ring(got), ring(o)), (name, vx, vy)  # out's ring is left as it was
        if name == "noise":
            assert (got[1:-1, 1:-1] != o[1:-1, 1:-1]).all()  # every interior cell was accumulated into
        assert same_bits(fu.download(), u), (name, vx, vy)


@pytest.mark.parametrize("nx,ny,dx,dy", CASES, ids=CASE_IDS)
def test_fused_step_is_copy_diffusion_advection(csim, nx, ny, dx, dy):
    fu, fo = csim.Field(nx, ny, 1, dx, dy), csim.Field(nx, ny, 1, dx, dy)
    for (name, u), (vx, vy) in itertools.product(fields(nx, ny), VELOCITIES):
        fu.upload(u)
        fo.fill(SENTINEL)
        csim.fused_step(fu, fo, D, DT, vx, vy)
        got = fo.download()
        want = u.copy()  # std::copy, then the two operators (reference src/main.cpp:104-107)
        ora.diffusion_step(u, want, dx, dy, D, DT)
        ora.advection_step(u, want, dx, dy, vx, vy, DT)
        assert same_cells(got, want), (name, vx, vy)
        assert same_bits(ring(got), ring(u)), (name, vx, vy)
        assert same_bits(fu.download(), u), (name, vx, vy)


def bc_field(nx, ny):
    """noise with a NaN and an Inf in interior cells that Neumann sides copy into the ring"""
    u = noise(nx, ny, 4)
    u[1, 1] = np.nan
    u[ny, nx] = np.inf
    return u


def check_boundary(csim, f, u, mix, phys, value):
    f.upload(u)
    csim.apply_boundary(f, csim.bc_codes(mix), phys, value)
    want = u.copy()
    ora.apply_boundary(want, ora.bc_codes(mix), phys, value)
    got = f.download()
    assert same_bits(got, want), (mix, phys, value, np.argwhere(got.view(np.int64) != want.view(np.int64))[:8].tolist())
    return want


@pytest.mark.parametrize("nx,ny", BC_SHAPES, ids=[f"{nx}x{ny}" for nx, ny in BC_SHAPES])
def test_apply_boundary_every_mix(csim, nx, ny):
    """all 81 mixes of Dirichlet / Neumann / Periodic with four physical sides, corners included"""
    f, u = csim.Field(nx, ny), bc_field(nx, ny)
    for mix, value in itertools.product(BC_MIXES, BC_VALUES):
        want = check_boundary(csim, f, u, mix, (1, 1, 1, 1), value)
        assert same_bits(want[1:-1, 1:-1], u[1:-1, 1:-1])
        if mix == "pppp":
            assert same_bits(want, u)  # apply_boundary leaves periodic sides to the halo exchange


@pytest.mark.parametrize("nx,ny", BC_SHAPES, ids=[f"{nx}x{ny}" for nx, ny in BC_SHAPES])
def test_apply_boundary_every_physical_mask(csim, nx, ny):
    """all 16 is_physical masks: a side with a neighbour keeps its ghost line"""
    f, u = csim.Field(nx, ny), bc_field(nx, ny)
    for mix, phys, value in itertools.product(MASK_MIXES, itertools.product((0, 1), repeat=4), BC_VALUES):
        want = check_boundary(csim, f, u, mix, phys, value)
        if phys == (0, 0, 0, 0):
            assert same_bits(want, u)


@pytest.mark.parametrize("nx,ny", [(257, 3), (3, 700)], ids=["257x3", "3x700"])
def test_fill_copy_swap(csim, nx, ny):
    u, v = planted(nx, ny, 5), noise(nx, ny, 6)
    a, b = csim.Field(nx, ny).upload(u), csim.Field(nx, ny).upload(v)
    for value in (2.5, -0.0, np.inf, 5e-324):
        b.fill(value)
        assert same_bits(b.download(), np.full_like(u, value)), value  # the ghosts are filled too
        assert same_bits(b.download_interior(), np.full((ny, nx), value)), value
    b.fill(np.nan)
    assert np.isnan(b.download()).all()
    assert same_bits(a.download(), u)
    b.copy_from(a)
    assert same_bits(b.download(), u) and same_bits(a.download(), u)
    b.upload(v)
    a.swap(b)
    assert same_bits(a.download(), v) and same_bits(b.download(), u)
    # the swapped fields keep working as operands: reductions and operators see the swapped contents
    assert a.minmax() == (v.min(), v.max())
    with np.errstate(all="ignore"):
        want = float(np.abs(v - u)[1:-1, 1:-1].max())
    got = a.linf_diff(b)
    assert np.isnan(got) if np.isnan(want) else got == want
    a.swap(b)
    assert same_bits(a.download(), u) and same_bits(b.download(), v)
    c = csim.Field(nx, ny)
    c.fill(SENTINEL)
    csim.diffusion_step(b, c, D, DT)
    want = np.full_like(v, SENTINEL)
    ora.diffusion_step(v, want, 1.0, 1.0, D, DT)
    assert same_bits(c.download(), want)
