"""tests/virtual_fuzz_cases.py — the seeded cases of the decomposed-run fuzz (tests/test_gpu_virtual_fuzz.py): process
grids of 2 .. 16 virtual ranks (tests/virtual_ranks.py) against the oracle.

`fuzz_cases(seed, per_world)` and `SEAMS` are pure: the GPU test runs them, and tests/test_virtual_fuzz_cases_host.py
checks on the CPU which tiles, sides, pass depths and caps they reach.  `tiles`, `fuse_limit` and `schedule` restate
csim_decomp_init, csim_stepper_fuse_limit of a multi-rank stepper and VirtualRanks.advance for that coverage check;
the host test holds `tiles` against the library and the oracle, the GPU test holds `fuse_limit` against the steppers."""
import numpy as np

from ensemble_fuzz_cases import DT_FRACTION, SPACINGS, STRIDE, VALUES, VX_SET, VY_SET, _pick, div_mode  # noqa: F401
from oracle import cpu_oracle as ora

DEFAULT_SEED = 20261019
# cases per world size, set from a measurement on an MI355X: thirty cases of 16 ranks, the slowest world size, take
# 2.0 s (12 ranks 1.5 s, 9 ranks 1.1 s, the others under a second); the host coverage conditions hold from 8 on
FUZZ_PER_WORLD = 30
WORLDS = [2, 3, 4, 5, 6, 7, 8, 9, 12, 16]
D_SET = [0.0, 0.01, 0.05, 0.2]
FUSES = [None, 0, 2, 3, 4, 5, 6, 7]
MAX_CELLS = 600_000
AUTO_DEPTH = 6   # pref_fuse of a multi-rank stepper (internal.hpp): the mid-size table at every tile size
MAX_FUSE = 7


def grid_dims(world):
    """csim_decomp_init: the most balanced factor pair, larger factor first"""
    small = max(f for f in range(1, world + 1) if f * f <= world and world % f == 0)
    return world // small, small


def tiles(world, nx, ny):
    """every rank's tile as oracle.cpu_oracle.decomp gives it: the last tile of an axis takes the remainder"""
    px, py = grid_dims(world)
    bx, by = nx // px, ny // py
    out = []
    for r in range(world):
        cx, cy = r // py, r % py
        out.append(dict(dims0=px, dims1=py, cx=cx, cy=cy,
                        left=(cx - 1) * py + cy if cx > 0 else -1, right=(cx + 1) * py + cy if cx + 1 < px else -1,
                        down=cx * py + cy - 1 if cy > 0 else -1, up=cx * py + cy + 1 if cy + 1 < py else -1,
                        nx_local=bx + (nx % px if cx == px - 1 else 0), ny_local=by + (ny % py if cy == py - 1 else 0),
                        x_offset=cx * bx, y_offset=cy * by))
    return out


def tile_cap(c):
    """(smallest tile extent in x, in y) of the case's decomposition; the smaller one caps the pass depth"""
    px, py = grid_dims(c["world"])
    return c["nx"] // px, c["ny"] // py


def fuse_limit(c):
    """csim_stepper_fuse_limit of the case's steppers: the depth asked for (option "fuse", 6 when left alone), at most
    the smallest tile extent and 7; 1 = single steps only"""
    depth = min(AUTO_DEPTH if c["fuse"] is None else c["fuse"], MAX_FUSE, *tile_cap(c))
    return depth if depth >= 2 else 1


def schedule(c):
    """the steps per pass of VirtualRanks.advance over the case's calls, one list per call (1 = a single step)"""
    depth, out = fuse_limit(c), []
    for n in c["calls"]:
        passes, remaining = [], n
        while remaining >= 3 and depth >= 2:
            t = min(depth, remaining - 1)
            passes.append(t)
            remaining -= t
        out.append(passes + [1] * remaining)
    return out


def time_step(dx, dy, D, vx, vy, fraction):
    return fraction * min(ora.safe_dt(dx, dy, vx, vy, D), 0.25)


def _split(rng, steps):
    if steps >= 2 and rng.random() < 0.5:
        a = int(rng.integers(1, steps))
        return [a, steps - a]
    return [steps]


def fuzz_cases(seed=DEFAULT_SEED, per_world=FUZZ_PER_WORLD):
    rng = np.random.default_rng(seed)
    cases = []
    for case in range(per_world * len(WORLDS)):
        world = WORLDS[case % len(WORLDS)]
        px, py = grid_dims(world)
        shape = (case // len(WORLDS)) % 4
        if shape == 0:      # two to four strips and a bit
            tw = int(rng.integers(113, 481))
        elif shape == 1:    # narrow
            tw = int(rng.integers(2, 10))
        else:
            tw = int(rng.integers(2, 301))
        th = int(rng.integers(2, 101))
        if case % 7 == 3:   # the smallest tile caps the pass depth (or just does not), by x or by y
            if rng.random() < 0.5:
                tw = int(rng.integers(2, 8))
            else:
                th = int(rng.integers(2, 8))
        th = max(2, min(th, MAX_CELLS // (px * tw * py)))
        # every other case: a remainder for the last tile of the axis
        nx = px * tw + (int(rng.integers(0, px)) if rng.random() < 0.5 else 0)
        ny = py * th + (int(rng.integers(0, py)) if rng.random() < 0.5 else 0)
        dx, dy = _pick(rng, SPACINGS)
        bc = "".join(_pick(rng, "dnp") for _ in range(4))
        D, vx, vy = _pick(rng, D_SET), _pick(rng, VX_SET), _pick(rng, VY_SET)
        dt = time_step(dx, dy, D, vx, vy, _pick(rng, DT_FRACTION))
        steps = int(rng.integers(0, 3)) if case % 11 == 4 else int(rng.integers(0, 31))
        opts = dict(rows_per_chunk=_pick(rng, [0, 1, 2, 5, 13]), xcd_swizzle=int(rng.integers(2)),
                    tail_split=int(rng.integers(3)), fused_2c=_pick(rng, [1, 1, 0]), pow2_v=_pick(rng, [2, 1]))
        cases.append(dict(case=case, world=world, nx=nx, ny=ny, dx=dx, dy=dy, bc=bc, value=_pick(rng, VALUES), D=D, vx=vx,
                          vy=vy, dt=dt, steps=steps, calls=_split(rng, steps), fuse=_pick(rng, FUSES), opts=opts,
                          field_seed=int(rng.integers(1 << 31))))
    return cases


def initial_interior(c):
    """the global interior (ny, nx) a case starts from: standard normal; "screened" cases: positive, with the case's
    blocks (x0, x1, y0, y1, factor) scaled — a factor of -0.0 leaves a block of -0.0"""
    u = np.random.default_rng(c["field_seed"]).standard_normal((c["ny"], c["nx"]))
    if c.get("field") == "screened":
        u = np.abs(u) + 0.5
        for x0, x1, y0, y1, factor in c["blocks"]:
            u[y0:y1, x0:x1] *= factor
    return u


def describe(c):
    """a case without its field, for failure messages"""
    return {k: v for k, v in c.items() if k != "blocks"}


# ---- the fixed seam cases -------------------------------------------------------------------------------------------
SEAM_BCS = ["dddd", "nnnn", "dnpd", "pdnp", "npdn", "pppp", "ndpn"]
SEAM_SPACINGS = [(1.0, 1.0), (0.5, 0.25), (0.7, 1.3)]           # division modes 0, 1, 2
SEAM_VELOCITIES = [(0.5, 0.25), (-0.5, -0.25), (0.5, -0.25), (-0.5, 0.25), (0.5, 0.0), (-1.0, 0.0), (0.0, 0.25),
                   (0.0, -0.25), (0.0, 0.0), (-0.0, 0.75), (0.25, -0.0)]   # the nine upwind sign classes, -0.0 twice
SEAM_ROWS = 5   # rows_per_chunk: even the small seam tiles have several chunks


def _seam(seams, world, nx, ny, fuse, what, **over):
    """one entry; BC mix, spacing class, velocity sign class, Dirichlet value, D, dt fraction, pow2_v and the split of
    the advance cycle with the entry's position, each with a period of its own; `over` fixes what the entry is about.
    steps = fuse + 3: one pass of the depth (or of the cap below it), one of two steps, one single step"""
    i = len(seams)
    px, py = grid_dims(world)
    assert nx * ny <= MAX_CELLS and nx // px >= 2 and ny // py >= 2, (what, world, nx, ny)
    c = dict(case=f"seam{i}", what=what, world=world, nx=nx, ny=ny, bc=SEAM_BCS[i % len(SEAM_BCS)],
             value=VALUES[(i // 3) % len(VALUES)], D=D_SET[i % len(D_SET)], fuse=fuse, field_seed=1000 + i,
             opts=dict(rows_per_chunk=SEAM_ROWS, xcd_swizzle=1, tail_split=1, fused_2c=1, pow2_v=[2, 1][i % 2]))
    c["dx"], c["dy"] = SEAM_SPACINGS[i % len(SEAM_SPACINGS)]
    c["vx"], c["vy"] = SEAM_VELOCITIES[i % len(SEAM_VELOCITIES)]
    opts = over.pop("opts", {})
    c.update(over)
    c["opts"].update(opts)
    depth = min(fuse, MAX_FUSE, nx // px, ny // py)
    c.setdefault("steps", depth + 3)
    c["dt"] = time_step(c["dx"], c["dy"], c["D"], c["vx"], c["vy"], DT_FRACTION[(i // 2) % len(DT_FRACTION)])
    # every fourth entry in two calls: the pass and a single step, then two single steps
    c["calls"] = [depth + 1, c["steps"] - depth - 1] if i % 4 == 1 and c["steps"] == depth + 3 else [c["steps"]]
    seams.append(c)
    return c


def _screened(seams, world, nx, ny, fuse, vel, pow2_v, fused_2c):
    """a positive field whose centre tile (two / four neighbour sides, four strips) carries a block of -0.0 and one of
    1e-250, and whose last tile one of 1e-250: tiles that pass the screens of the fast bodies, and tiles that fall back"""
    dx, dy = SEAM_SPACINGS[len(seams) % 2]   # the screened 12-operation body needs division mode 0 or 1
    t = tiles(world, nx, ny)
    mid, last = t[world // 2], t[-1]
    blocks = []
    for tile, col, factor in ((mid, 130, -0.0), (mid, 250, 1e-250), (last, 130, 1e-250)):
        x0, y0 = tile["x_offset"] + col, tile["y_offset"] + tile["ny_local"] // 2 - 3
        blocks.append((x0, x0 + 20, y0, y0 + 6, factor))
    _seam(seams, world, nx, ny, fuse, "screened bodies on tiles with stored deep halos", dx=dx, dy=dy, vx=vel[0],
          vy=vel[1], D=0.05, bc="dnpd", field="screened", blocks=blocks,
          opts=dict(rows_per_chunk=6, pow2_v=pow2_v, fused_2c=fused_2c))


def _build_seams():
    seams = []
    # tile widths at the strip seams of depth T, on 2 x 2 (corner tiles) and 3 x 1 (a middle tile), equal and unequal
    heights = 0
    for T in (4, 6, 7):
        S = STRIDE[T]
        for w in (S - 1, S, S + 1, 2 * S, 2 * S + 1, 128, 129, 3 * S + 5):
            for world in (4, 3):
                px, py = grid_dims(world)
                for extra in (0, 1):
                    h = [T - 1, T, T + 1, 2 * T - 2, 13, 25, 40][heights % 7]
                    heights += 1
                    _seam(seams, world, px * w + extra, py * h, T, f"width {w}{'+1' if extra else ''} at depth {T}")
    # 3 x 3: a centre tile with eight distinct peers, edge tiles with three neighbour sides
    for (nx, ny), shift in (((1001, 203), 0), ((375, 91), 1)):
        for k, T in enumerate((2, 5, 7)):
            _seam(seams, 9, nx, ny, T, "3 x 3", bc=["nnnn", "dnpd", "pdnp"][(k + shift) % 3])
    _seam(seams, 12, 1000, 90, 7, "4 x 3")
    _seam(seams, 16, 1000, 100, 7, "4 x 4")
    for world, nx, ny in ((5, 17, 30), (5, 1160, 30), (7, 23, 12), (7, 900, 40)):
        _seam(seams, world, nx, ny, 7, "chain")
    # the smallest tile caps the pass depth; fuse = 7, so a pass of exactly the cap runs
    for world, nx, ny in ((8, 20, 40), (4, 9, 30), (9, 15, 9), (6, 12, 7), (4, 8, 4),           # caps 5x 4x 3y 3y 2y
                          (2, 4, 12), (3, 9, 10), (4, 30, 8), (8, 40, 10), (2, 12, 20), (4, 26, 12)):  # 2x 3x 4y 5y 6x 6y
        c = _seam(seams, world, nx, ny, 7, "capped depth")
        c["cap"] = min(tile_cap(c))
    # screened bodies: the middle tile of 3 x 1 and the centre of 3 x 3, four strips each
    runs = [((0.5, 0.25), 1, 1), ((-0.5, -0.25), 1, 1), ((0.5, 0.25), 0, 1), ((-0.5, -0.25), 1, 0), ((0.5, 0.0), 1, 1),
            ((0.0, 0.0), 1, 1), ((0.0, 0.0), 1, 0)]
    for world, nx, ny in ((3, 1080, 80), (9, 1080, 120)):
        for k, (vel, pow2_v, fused_2c) in enumerate(runs):
            _screened(seams, world, nx, ny, 6 + k % 2, vel, pow2_v, fused_2c)
    return seams


SEAMS = _build_seams()
