"""Nonzero Dirichlet values through the single stepper (csim_stepper_create's bc_value).  The reference driver always
passes 0.0 to apply_boundary, and the device buffers start zero-filled, so a path that wrote 0 instead of the value
(the ghost fill, the deep ghost layers of decomposed tiles, the multi-step sweep's edge bodies, the closing FinLines
fill) would pass every run with the value 0.  Compared BIT for bit (integer views: +0 and -0 differ; NaN cells by
position) with the value-aware oracle, which tests/test_oracle_golden.py pins to the compiled reference
(tests/golden/dirichlet_value.npz), ghost ring included."""
import json
import os

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cpu_oracle as ora
from test_gpu_comm import self_neighbor_decomp
from test_gpu_diffusion_only import nasty_field, same_bits
from test_gpu_parity import VARIANT_CFGS
from virtual_ranks import VirtualRanks, tile_mask

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "dirichlet_value.npz")


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


@pytest.fixture(scope="module")
def fixture():
    z = np.load(FIXTURE, allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def with_ghosts(interior):
    ny, nx = interior.shape
    f = np.zeros((ny + 2, nx + 2))
    f[1:-1, 1:-1] = interior
    return f


def stepper_run(csim, u0, dx, dy, D, vx, vy, dt, bc, value, calls, opts=None):
    ny, nx = u0.shape[0] - 2, u0.shape[1] - 2
    st = csim.Stepper.single(nx, ny, dx, dy, bc, value)
    for k, v in (opts or {}).items():
        st.set_option(k, v)
    st.upload(u0)
    for n in calls:
        st.run(D, dt, vx, vy, n)
    out = st.download()
    st.close()
    return out


def test_fixture_cases_every_variant_and_split(csim, fixture):
    z, cases = fixture
    for c in cases:
        k = c["idx"]
        dt = float(z[f"c{k}_dt_effective"])
        u0 = with_ghosts(z[f"c{k}_u0"])
        want = z[f"c{k}_local_np1_rank0"]
        args = (c["dx"], c["dy"], c["D"], c["vx"], c["vy"], dt, csim.bc_codes(c["bc"]), c["bc_value"])
        for opts in VARIANT_CFGS:
            got = stepper_run(csim, u0, *args, [c["steps"]], opts)
            assert same_bits(got, want), (c["name"], opts)
        for calls in ([1, 2, c["steps"] - 3], [5, c["steps"] - 5], [1] * c["steps"]):
            got = stepper_run(csim, u0, *args, calls)
            assert same_bits(got, want), (c["name"], calls)


SWEEP_VALUES = [1.5, -3.25, -0.0, 1e-310, 7e307, np.inf, np.nan]
SWEEP_SPACINGS = [(1.0, 1.0), (0.5, 0.25), (0.7, 1.3)]


def test_seeded_sweep_vs_oracle(csim):
    """BC mixes with 1-4 Dirichlet sides, the three division modes, every pass depth, values from -0 and subnormal to
    near overflow, Inf and NaN, random uploaded ghost rings: a Dirichlet side takes the value, a Periodic one keeps
    its ring"""
    rng = np.random.default_rng(int(os.environ.get("CSIM_FUZZ_SEED", "20261016")))
    for case in range(210):
        nd = 1 + case % 4
        kinds = ["d"] * nd + [str(rng.choice(list("np"))) for _ in range(4 - nd)]
        bcs = "".join(rng.permutation(kinds))
        dx, dy = SWEEP_SPACINGS[case % 3]
        value = SWEEP_VALUES[(case // 3) % len(SWEEP_VALUES)]
        fuse = int(rng.choice([-1, 0, 2, 3, 4, 5, 6, 7]))
        nx = int(rng.integers(1, 300)) if case % 5 else int(rng.integers(120, 700))
        ny = int(rng.integers(1, 120))
        D = float(rng.choice([0.0, 0.01, 0.05, 0.2]))
        vx = float(rng.choice([0.0, 0.5, -0.5, 0.25]))
        vy = float(rng.choice([0.0, 0.25, -0.25, -0.75]))
        dt = 0.8 * min(0.1, ora.safe_dt(dx, dy, vx, vy, D)) if (D or vx or vy) else 0.1
        steps = int(rng.integers(1, 25))
        calls = [steps]
        if steps >= 3 and case % 2:
            a = int(rng.integers(1, steps - 1))
            calls = [a, steps - a]
        u0 = rng.standard_normal((ny + 2, nx + 2))
        want = u0.copy()
        bc = ora.bc_codes(bcs)
        with np.errstate(all="ignore"):
            ora.run_single(want, dx, dy, D, vx, vy, dt, bc, steps, value=value)
        got = stepper_run(csim, u0, dx, dy, D, vx, vy, dt, bc, value, calls, dict(fuse=fuse))
        what = (case, nx, ny, dx, dy, D, vx, vy, bcs, value, fuse, calls)
        assert same_bits(got, want), what
        lines = [got[1:-1, 0], got[1:-1, -1], got[0, 1:-1], got[-1, 1:-1]]
        ring0 = [u0[1:-1, 0], u0[1:-1, -1], u0[0, 1:-1], u0[-1, 1:-1]]
        for s, code in enumerate(bc):
            if code == ora.DIRICHLET:
                assert same_bits(lines[s], np.full(lines[s].shape, value)), (what, s)
            elif code == ora.PERIODIC:
                assert same_bits(lines[s], ring0[s]), (what, s)


@pytest.mark.parametrize("dx,dy", [(1.0, 1.0), (0.5, 2.0)])
@pytest.mark.parametrize("value", [1.5, -0.0])
def test_zero_velocity_flavour(csim, dx, dy, value):
    """vx = vy = 0: the screened seven-operation interior body, next to Dirichlet ghosts holding the value"""
    nx, ny, D = 700, 160, 0.05
    dt = min(0.1, csim.safe_dt(dx, dy, 0.0, 0.0, D))
    for bcs in ("dddd", "dndp"):
        u0 = nasty_field(nx, ny, 61, nonfinite=False)
        bc = csim.bc_codes(bcs)
        for fuse, steps in [(2, 5), (4, 7), (7, 10), (-1, 17)]:
            want = u0.copy()
            ora.run_single(want, dx, dy, D, 0.0, 0.0, dt, bc, steps, value=value)
            for on in (1, 0):
                st = csim.Stepper.single(nx, ny, dx, dy, bc, value)
                for k, v in dict(fuse=fuse, rows_per_chunk=18, fused_2c=on).items():
                    st.set_option(k, v)
                st.upload(u0)
                st.run(D, dt, 0.0, 0.0, steps)
                assert st.get_option("diffusion_only_active") == on
                got = st.download()
                st.close()
                assert same_bits(got, want), (bcs, fuse, on)


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("world", [4, 8])
def test_virtual_ranks_against_the_fixture(csim, fixture, world, depth):
    """decomposed tiles (external-halo steppers, faces routed in this process): Dirichlet physical sides, their deep
    ghost layers and the closing fill, against the reference's own per-rank arrays under mpirun"""
    z, cases = fixture
    used = 0
    for c in cases:
        if world not in c["ranks"]:
            continue
        used += 1
        k = c["idx"]
        dt = float(z[f"c{k}_dt_effective"])
        vr = VirtualRanks(csim, world, c["nx"], c["ny"], c["dx"], c["dy"], csim.bc_codes(c["bc"]), c["bc_value"],
                          fuse=depth)
        try:
            for r, dec in enumerate(vr.decs):
                assert list(dec.as_dict().values()) == list(z[f"c{k}_decomp_np{world}"][r])
            vr.upload_global(z[f"c{k}_u0"])
            vr.advance(c["D"], dt, c["vx"], c["vy"], c["steps"], depth=depth)
            for r, dec in enumerate(vr.decs):
                got, want = vr.download(r), z[f"c{k}_local_np{world}_rank{r}"]
                mask = tile_mask(dec)   # the reference leaves multi-rank corner ghosts undefined
                assert same_bits(got[mask], want[mask]), (c["name"], world, depth, r)
        finally:
            vr.close()
    assert used >= (1 if world == 8 else 2)


def torus_oracle_value(u0, dx, dy, D, vx, vy, dt, steps, sides, bc, value):
    """tests/test_gpu_comm.py's torus_oracle with a Dirichlet value on the physical sides"""
    u, tmp = u0.copy(), u0.copy()
    phys = [0 if s else 1 for s in sides]
    for _ in range(steps):
        if sides[0]:
            u[1:-1, 0] = u[1:-1, -2]
        if sides[1]:
            u[1:-1, -1] = u[1:-1, 1]
        if sides[2]:
            u[0, 1:-1] = u[-2, 1:-1]
        if sides[3]:
            u[-1, 1:-1] = u[1, 1:-1]
        ora.step_tile(u, tmp, dx, dy, D, vx, vy, dt, bc, phys, value)
        u, tmp = tmp, u
    return u


@pytest.mark.parametrize("sides,bc", [((1, 1, 0, 0), "dddn"), ((0, 0, 1, 1), "dndd")])
@pytest.mark.parametrize("overlap", [0, 1, 3, 4, 5])
def test_self_linked_tile_with_dirichlet_value(csim, sides, bc, overlap):
    """the exchange path (a tile linked to itself through RCCL) next to physical Dirichlet sides: every exchange
    schedule, including the bulk-first runs and their one-off ghost fill, the halo extension of the physical edges
    and the closing FinLines fill"""
    nx, ny, steps, value = 1160, 300, 18, -3.25
    D, vx, vy, dt = 0.05, 0.5, -0.25, 0.1
    rng = np.random.default_rng(29)
    u0 = np.zeros((ny + 2, nx + 2))
    u0[1:-1, 1:-1] = rng.standard_normal((ny, nx))
    codes = csim.bc_codes(bc)
    want = torus_oracle_value(u0, 1.0, 1.0, D, vx, vy, dt, steps, sides, codes, value)
    st = csim.Stepper(self_neighbor_decomp(csim, nx, ny, sides), 1.0, 1.0, codes, value)
    st.comm_init(csim.comm_unique_id())
    st.set_option("overlap", overlap)
    st.set_option("fuse", 6)
    st.upload(u0)
    st.run(D, dt, vx, vy, 7)
    st.run(D, dt, vx, vy, steps - 7)
    got = st.download()
    st.close()
    mask = np.ones(got.shape, bool)
    mask[[0, 0, -1, -1], [0, -1, 0, -1]] = False   # corners are never exchanged
    assert same_bits(got[mask], want[mask])
