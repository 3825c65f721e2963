"""The batched stepper (csim_ensemble_*) beyond its hand-picked cases: a seeded fuzz over member counts, shapes, the
three division modes, BC mixes, per-member physics, split runs, options and Dirichlet values
(tests/ensemble_fuzz_cases.py; what it reaches is checked on the CPU by tests/test_ensemble_fuzz_host.py), then the
screens per member, changes between runs, the chunk heights of the multi-step sweep and the member limit.  Every member
must equal oracle.cpu_oracle.run_single with its own parameters, BIT for bit (integer views, NaN cells by position),
whole array, ghost ring included."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from ensemble_fuzz_cases import CHUNK_CASES, DEFAULT_SEED, fuzz_cases, fuzz_fields
from oracle import cpu_oracle as ora
from test_gpu_diffusion_only import nasty_field, same_bits
from test_gpu_ensemble import PHYS12, assert_members, csim, oracle_runs, random_fields  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


def set_phys(e, phys):
    e.set_physics(*[[p[k] for p in phys] for k in range(4)])


def test_fuzz_members_equal_the_oracle(csim):
    seed = int(os.environ.get("CSIM_FUZZ_SEED", DEFAULT_SEED))   # (other seeds: extended soak runs)
    for c in fuzz_cases(seed):
        u0s = fuzz_fields(c)
        bc = csim.bc_codes(c["bc"])
        e = csim.Ensemble(c["B"], c["nx"], c["ny"], c["dx"], c["dy"], bc, c["value"])
        e.set_option("fuse", c["fuse"])
        e.set_option("fused_2c", c["fused_2c"])
        e.upload_all(u0s)
        set_phys(e, c["phys"])
        for n in c["calls"]:
            e.run(n)
        got = e.download_all()
        e.close()
        want = oracle_runs(u0s, c["phys"], bc, c["steps"], c["dx"], c["dy"], c["value"])
        bad = [k for k in range(c["B"]) if not same_bits(got[k], want[k])]
        assert not bad, ({k: v for k, v in c.items() if k != "phys"}, bad, [c["phys"][k] for k in bad[:4]])


# one member per upwind-sign class (3 * cx + cy, per axis 0: v < 0, 1: v > 0, 2: v == 0), then a wildly unstable one
# with zero velocity: its screen threshold is 0, so it runs in class 4 next to the stable member there
CLASS_PHYS = [(0.05, 0.1, -0.5, -0.25), (0.05, 0.1, -0.5, 0.25), (0.05, 0.1, -0.5, 0.0),
              (0.05, 0.1, 0.5, -0.25), (0.05, 0.1, 0.5, 0.25), (0.05, 0.1, 0.5, 0.0),
              (0.05, 0.1, 0.0, -0.25), (0.05, 0.1, 0.0, 0.25), (0.1, 0.1, 0.0, 0.0)]
UNSTABLE = (3.0e18, 1.0, 0.0, 0.0)


@pytest.mark.parametrize("nx", [700, 701])
@pytest.mark.parametrize("dx,dy", [(1.0, 1.0), (0.5, 2.0), (0.7, 1.3)])
@pytest.mark.parametrize("fused_2c", [1, 0])
def test_screens_per_member(csim, nx, dx, dy, fused_2c):
    """nasty fields (around the overflow screen, +-Inf, NaN, -0 blocks, subnormals) in a member of every sign class,
    clean ones beside them in the same classes: every member is the oracle's, and the clean members come out exactly
    as in a run without the nasty ones"""
    ny, steps = 160, 9
    bc = csim.bc_codes("dnpd")
    phys = CLASS_PHYS + CLASS_PHYS + [UNSTABLE]
    if fused_2c and (dx, dy) == (1.0, 1.0):
        assert [csim.ensemble_sign_class(*p) for p in CLASS_PHYS] == list(range(9))
        assert csim.ensemble_sign_class(*UNSTABLE) == 4
    nasty = list(range(len(CLASS_PHYS)))
    clean = random_fields(len(phys), nx, ny, seed=nx + 7 * fused_2c)
    mixed = clean.copy()
    for k in nasty:
        mixed[k] = nasty_field(nx, ny, 100 + k)
    runs = []
    for u0s in (mixed, clean):
        e = csim.Ensemble(len(phys), nx, ny, dx, dy, bc)
        e.set_option("fused_2c", fused_2c)
        e.upload_all(u0s)
        set_phys(e, phys)
        e.run(steps)
        runs.append(e.download_all())
        e.close()
    assert_members(runs[0], oracle_runs(mixed, phys, bc, steps, dx, dy), f"{nx} {dx} {dy} fused_2c={fused_2c}")
    assert np.nanmax(np.abs(runs[0][-1])) > 1e100   # the unstable member did grow wildly
    for k in range(len(CLASS_PHYS), len(phys)):
        assert same_bits(runs[0][k], runs[1][k]), f"clean member {k} depends on the nasty members"


@pytest.mark.parametrize("bcs,value,dx,dy", [("dnpd", 1.5, 1.0, 1.0), ("pppp", 0.0, 0.5, 2.0),
                                            ("dnpd", -0.0, 0.7, 1.3), ("ndnd", -3.25, 0.5, 0.25)])
def test_changes_between_runs(csim, bcs, value, dx, dy):
    """physics changed between calls (signs flipped, a component zeroed, dt changed: members change sign class),
    fused_2c toggled, one member uploaded anew: after every call each member is the oracle run over the same sequence"""
    nx, ny, B = 131, 67, len(PHYS12)
    bc = csim.bc_codes(bcs)
    u0s = random_fields(B, nx, ny, seed=sum(map(ord, bcs)) + 17)
    flipped = [(D, 0.5 * dt, -vx, vy if k % 3 else 0.0) for k, (D, dt, vx, vy) in enumerate(PHYS12)]
    still = [(D, dt, vx if k % 2 else 0.0, 0.0) for k, (D, dt, vx, vy) in enumerate(PHYS12)]
    fresh = random_fields(1, nx, ny, seed=99)[0]
    script = [("run", 7), ("phys", flipped), ("run", 9), ("fused_2c", 0), ("run", 5), ("upload", 3), ("run", 6),
              ("fused_2c", 1), ("phys", still), ("run", 11), ("phys", PHYS12), ("upload", 11), ("run", 3), ("run", 4)]
    e = csim.Ensemble(B, nx, ny, dx, dy, bc, value)
    e.upload_all(u0s)
    set_phys(e, PHYS12)
    want = [u.copy() for u in u0s]
    phys = PHYS12
    for op, arg in script:
        if op == "run":
            e.run(arg)
            want = oracle_runs(np.array(want), phys, bc, arg, dx, dy, value)
            assert_members(e.download_all(), want, f"{bcs} after {op} {arg}")
        elif op == "phys":
            phys = arg
            set_phys(e, phys)
        elif op == "fused_2c":
            e.set_option("fused_2c", arg)
        else:
            e.upload(arg, fresh)
            want[arg] = fresh.copy()
    e.close()


def _chunk_member(seed, k, nx, ny):
    return np.random.default_rng([seed, k]).standard_normal((ny + 2, nx + 2))


@pytest.mark.parametrize("B,nx,ny,steps", CHUNK_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in CHUNK_CASES])
def test_chunk_heights_one_sign_class(csim, B, nx, ny, steps):
    """every member in one sign class, so that one launch covers them all and the member count sets the chunk height
    (tall chunks for few members, the clip to ny on short grids): all checksums and a sample of whole arrays"""
    bc = csim.bc_codes("dnpd")
    rng = np.random.default_rng(B * 1000 + ny)
    phys = [(0.01 + 0.04 * rng.random(), 0.05 + 0.05 * rng.random(), 0.1 + 0.4 * rng.random(), 0.1 + 0.3 * rng.random())
            for _ in range(B)]
    assert {csim.ensemble_sign_class(*p) for p in phys} == {4}
    sample = sorted({0, 1, B // 3, B // 2, B - 1})
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, bc, 1.5)
    for k in range(B):
        e.upload(k, _chunk_member(B, k, nx, ny))
    set_phys(e, phys)
    e.run(steps)
    sums = e.checksums()
    got = {k: e.download(k) for k in sample}
    e.close()
    ora.lib()

    def one(k):
        u = _chunk_member(B, k, nx, ny)
        D, dt, vx, vy = phys[k]
        ora.run_single(u, 1.0, 1.0, D, vx, vy, dt, bc, steps, value=1.5)
        return csim.checksum_host(u[1:-1, 1:-1]), (u if k in got else None)
    with ThreadPoolExecutor(8) as ex:
        want = list(ex.map(one, range(B)))
    bad = [k for k in range(B) if sums[k] != want[k][0]]
    assert not bad, f"checksums of members {bad[:10]} differ ({len(bad)} of {B})"
    for k in sample:
        assert same_bits(got[k], want[k][1]), f"member {k}"


def test_member_limit(csim):
    """65535 members (grid.y of the step, ghost and reduction launches) on a grid that still takes the multi-step pass;
    one more is refused"""
    B, nx, ny, steps = 65535, 6, 5, 9
    with pytest.raises(csim.CsimError) as ex:
        csim.Ensemble(B + 1, nx, ny)
    assert ex.value.code == 1
    assert csim.ensemble_plan(steps, nx, ny)[1] >= 1
    bc = csim.bc_codes("dnpd")
    phys = [PHYS12[k % len(PHYS12)] for k in range(B)]
    u0s = random_fields(B, nx, ny, seed=65535)
    e = csim.Ensemble(B, nx, ny, 1.0, 1.0, bc, -3.25)
    e.upload_all(u0s)
    set_phys(e, phys)
    e.run(steps)
    assert e.get_option("depth_used") > 1
    got = e.download_all()
    sums = e.checksums()
    e.close()
    want = oracle_runs(u0s, phys, bc, steps, value=-3.25)
    assert_members(got, want, "65535 members")
    assert not same_bits(got[-1], u0s[-1])
    assert sums[-1] == csim.checksum_host(want[-1][1:-1, 1:-1])
