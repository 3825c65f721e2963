"""tests/ensemble_fuzz_cases.py — the seeded cases of the batched stepper's fuzz (tests/test_gpu_ensemble_fuzz.py).

`fuzz_cases(seed, n)` is a pure function of its arguments: the GPU test steps these cases, and
tests/test_ensemble_fuzz_host.py checks on the CPU which paths of csim_ensemble_run they reach.  `chunk_rows`
restates the chunk-height choice of ens_sweepO_div (ensemble.hip) for that coverage check only; no GPU assertion
depends on it."""
import numpy as np

from oracle import cpu_oracle as ora

DEFAULT_SEED = 20261016
FUZZ_CASES = 300

SPACINGS = [(1.0, 1.0), (0.5, 0.25), (2.0, 0.5), (0.7, 1.3), (1.0, 0.3)]  # as the single stepper's fuzz
D_SET = [0.0, 0.0, 0.01, 0.05, 0.2]
VX_SET = [0.0, -0.0, 0.5, -0.5, 0.25, -1.0]
VY_SET = [0.0, -0.0, 0.25, -0.25, 0.75]
DT_FRACTION = [0.8, 0.5, 0.2]
VALUES = [0.0, 1.5, -0.0]
# output columns per strip of the multi-step sweep at pass depth T (OverlapGeom<T>::STRIDE, sweep_core.hpp)
STRIDE = {2: 124, 3: 120, 4: 120, 5: 116, 6: 116, 7: 112}


def _pick(rng, values):
    return values[int(rng.integers(len(values)))]


def member_phys(rng, dx, dy):
    """(D, dt, vx, vy) with dt <= 0.8 safe_dt (dt = 0.1 when nothing moves)"""
    D, vx, vy = _pick(rng, D_SET), _pick(rng, VX_SET), _pick(rng, VY_SET)
    lim = ora.safe_dt(dx, dy, vx, vy, D)
    dt = _pick(rng, DT_FRACTION) * min(lim, 0.25) if np.isfinite(lim) else 0.1
    return (D, dt, vx, vy)


def fuzz_cases(seed=DEFAULT_SEED, n=FUZZ_CASES):
    rng = np.random.default_rng(seed)
    cases = []
    for case in range(n):
        shape = case % 6
        if shape == 0:      # odd width, two strips or more: the right edge's odd col_case
            nx = 2 * int(rng.integers(61, 200)) + 1
        elif shape == 1:    # even width, two strips or more
            nx = 2 * int(rng.integers(61, 200))
        elif shape == 2:    # narrow: single steps only below the pass depth
            nx = int(rng.integers(1, 9))
        else:
            nx = int(rng.integers(1, 401))
        if case % 17 == 5:
            nx = int(rng.integers(400, 901))
        ny = int(rng.integers(1, 151))
        if case % 8 == 3:
            ny = int(rng.integers(1, 7))
        elif case % 23 == 7:
            ny = int(rng.integers(150, 401))
        B = int(rng.integers(25, 71)) if case % 9 == 4 else int(rng.integers(1, 25))
        B = max(1, min(B, 3_000_000 // (nx * ny)))
        dx, dy = _pick(rng, SPACINGS)
        bc = "".join(_pick(rng, "dnp") for _ in range(4))
        phys = [member_phys(rng, dx, dy) for _ in range(B)]
        steps = int(rng.integers(0, 31))
        calls = [steps]
        if steps >= 2 and rng.random() < 0.5:
            a = int(rng.integers(1, steps))
            calls = [a, steps - a]
        cases.append(dict(case=case, B=B, nx=nx, ny=ny, dx=dx, dy=dy, bc=bc, phys=phys, steps=steps, calls=calls,
                          fuse=_pick(rng, [-1, -1, -1, 0]), fused_2c=_pick(rng, [1, 1, 0]),
                          value=_pick(rng, VALUES), field_seed=int(rng.integers(1 << 31))))
    return cases


def fuzz_fields(c):
    """every member's initial array: random interior AND ghost ring (Periodic sides keep theirs)"""
    rng = np.random.default_rng(c["field_seed"])
    return rng.standard_normal((c["B"], c["ny"] + 2, c["nx"] + 2))


def div_mode(dx, dy):
    """make_phys (api.cpp): 0 unit spacing, 1 powers of two (exact reciprocals), 2 IEEE division"""
    def pow2(v):
        m, _ = np.frexp(v)
        return m == 0.5
    if dx == 1.0 and dy == 1.0:
        return 0
    return 1 if all(pow2(v) for v in (dx, dy, dx * dx, dy * dy)) else 2


def chunk_rows(count, nx, ny, T):
    """ens_sweepO_div's chunk height for a launch of `count` members (coverage aid only)"""
    nstrips = -(-nx // STRIDE[T])
    ry = 64
    while ry > 6 and count * nstrips * -(-ny // ry) < 8192:
        ry >>= 1
    ry = max(ry, 6)
    ry += (6 - (ry + 2 * (T - 1)) % 6) % 6
    return min(ry, ny)


# the targeted chunk-height cases of the GPU test: every member in one sign class; (members, nx, ny, steps) -> rows
CHUNK_CASES = [(32, 512, 512, 8), (64, 512, 512, 8), (128, 512, 512, 4), (1024, 256, 256, 4), (5, 40, 5, 9),
               (3, 200, 4, 7)]
