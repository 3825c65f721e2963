"""tests/held_seam_cases.py — the cases of the held-row seam test (tests/test_gpu_held_seams.py) for k_held_mv,
k_held_transform (csrc/ensemble_held.hip) and the ROWS form of k_obsgram_partial (csrc/ensemble_obsgram.hip): member
counts and observation counts that put the 64-row blocks, the four-output tail and the staging walks on their seams,
the inputs of a case, and the wrong kernels that the reference must tell from the right one.

`reaches` restates what a launch of a case does from the three constants below; CASES states the same by hand, and
tests/test_held_seam_cases_host.py holds the two against each other on the CPU.  No GPU assertion depends on `reaches`.
`inputs` builds everything a case uploads and everything it is compared with except the weights; `weights` adds the
ETKF's (W, wbar) in the order of a path.  `wrong_variants` builds, in plan order as the kernels see the rows, what five
subtly wrong kernels would leave behind.  numpy and the restatements only; the library is passed in for its host-only
helpers (taps, plan, weights)."""
import collections

import numpy as np

import etkf_restatement as etkf
import held_restatement as held
import obsnet_restatement as obsnet
import obsop_restatement as obsop
import screen_restatement as screen

HELD_ROWS = 64       # csrc/ensemble_held.hip:28, rows per workgroup of k_held_mv and k_held_transform
HELD_RB = 4          # csrc/ensemble_held.hip:30, outputs that share one pass over the members
GRAM_THREADS = 256   # csrc/gram_plan.hpp:27, lanes that stage a segment's run in the ROWS form
HELD_LD = 65         # csrc/ensemble_held.hip:29, doubles from one member to the next in the tile
MAX_MEMBERS = 256    # csrc/gram_plan.hpp:23

GRID = (16, 16, 1.0, 1.0, 2.5)   # nx, ny, dx, dy, loc: windows overlap, the plan has several levels
TOL = 3.0                        # the background check of the analyses
INFLATION = 1.1

Case = collections.namedtuple("Case", "M nobs truth kind path blocks last_rows r64 r256 r4 carry64 carry256")
Case.__doc__ = """M forecast members, nobs observations, the truth member's place (None, "first", "middle", "last"), the
network's kind and the paths ("host" or "both"); then what the launch reaches, typed in: workgroups of the held
kernels, rows of the last one, 64 % M, 256 % M, M % 4, and whether the carry branch of held_stage and of the ROWS
staging is taken"""

#        M  nobs  truth     kind        path   blocks last 64%M 256%M M%4 carry64 carry256
CASES = [
    Case(6, 1, None, "point", "both", 1, 1, 4, 4, 2, False, False),          # one row, 63 idle lanes
    Case(2, 129, "first", "point", "host", 3, 1, 0, 0, 2, False, False),     # smallest M, three blocks, a tail of one row
    Case(3, 65, "last", "bilinear", "both", 2, 1, 1, 1, 3, True, False),     # M < HELD_RB, the tail clamps twice; 192
    #                                                                          elements: one trip of the 256 lanes
    Case(7, 63, "middle", "box", "host", 1, 63, 1, 4, 3, True, True),        # one short of a block
    Case(7, 64, None, "point", "host", 1, 64, 1, 4, 3, True, True),          # exactly one full block
    Case(63, 65, "first", "point", "host", 2, 1, 1, 4, 3, True, True),       # just below a wave of members
    Case(64, 128, "middle", "point", "both", 2, 64, 0, 0, 0, False, False),  # dc = 1, dk = 0, two full blocks
    Case(65, 129, "last", "point", "both", 3, 1, 64, 61, 1, True, True),     # M > 64: dc = 0
    Case(129, 65, None, "point", "host", 2, 1, 64, 127, 1, True, True),
    Case(255, 65, "middle", "point", "host", 2, 1, 64, 1, 3, True, True),    # 256 % M = 1
    Case(256, 129, "last", "point", "both", 3, 1, 64, 0, 0, True, False),    # the largest LDS request, three blocks
]

DEVICE_REQUIRED = [(3, 65), (64, 128), (65, 129), (256, 129)]


def name(c):
    return f"M{c.M}_n{c.nobs}_t{c.truth}_{c.kind}"


def case_of(M, nobs):
    return next(c for c in CASES if (c.M, c.nobs) == (M, nobs))


# (case, device): every case on the host path, the "both" ones on the device path as well
RUNS = [(c, False) for c in CASES] + [(c, True) for c in CASES if c.path == "both"]
RUN_IDS = [f"{name(c)}_{'device' if d else 'host'}" for c, d in RUNS]


# ---- what a launch reaches, from the constants --------------------------------------------------------------------

def walk_carries(M, lanes, rows):
    """whether the walk `c += dc, k += dk; if (k >= M) k -= M, ++c` of a staging loop over a run of rows * M elements,
    `lanes` at a time, ever takes its branch: an emulation of every lane, which also holds the walk to e = c M + k"""
    dc, dk = lanes // M, lanes - (lanes // M) * M
    taken = False
    for lane in range(lanes):
        c, k = lane // M, lane % M
        e = lane
        while e < rows * M:
            assert (c, k) == (e // M, e % M), (M, lanes, e)
            c, k, e = c + dc, k + dk, e + lanes
            if k >= M:
                if e < rows * M:
                    taken = True
                k, c = k - M, c + 1
    return taken


def reaches(M, nobs):
    """(blocks, rows of the last block, 64 % M, 256 % M, M % 4, carry of held_stage, carry of the ROWS staging); a carry
    counts when some block (segment) of the launch takes it"""
    blocks = -(-nobs // HELD_ROWS)
    last = nobs - (blocks - 1) * HELD_ROWS
    sizes = {HELD_ROWS} if blocks > 1 else set()
    sizes.add(last)
    return (blocks, last, HELD_ROWS % M, GRAM_THREADS % M, M % HELD_RB,
            any(walk_carries(M, HELD_ROWS, n) for n in sizes), any(walk_carries(M, GRAM_THREADS, n) for n in sizes))


def held_lds_bytes(M):
    """the dynamic LDS of k_held_mv and k_held_transform (held_lds)"""
    return 8 * HELD_LD * M


# ---- the inputs of a case ------------------------------------------------------------------------------------------------

def truth_of(where, B):
    return {None: None, "first": 0, "middle": B // 2, "last": B - 1}[where]


def members(B, grid, seed):
    """members() of tests/test_gpu_held.py: every (member, cell) value is distinct"""
    nx, ny = grid[0], grid[1]
    rng = np.random.default_rng([seed, B, nx, ny])
    return 3.0 + rng.standard_normal((ny + 2, nx + 2))[None] + 0.5 * rng.standard_normal((B, ny + 2, nx + 2))


def linear_network(csim, rng, grid, kind, nobs):
    """make_network() of tests/test_gpu_held.py for its two linear kinds: bilinear stations between grid points with
    four on the sides, 3 x 3 footprints clipped at the sides with two on one cell"""
    nx, ny = grid[0], grid[1]
    r = rng.uniform(0.5, 2.0, nobs)
    if kind == "bilinear":
        x, y = rng.uniform(1, nx, nobs), rng.uniform(1, ny, nobs)
        x[:4], y[:4] = [1.0, nx, 1.25, nx - 0.5], [1.0, ny, ny - 0.25, 1.5]
        i, j, taps = csim.bilinear_taps(nx, ny, x, y)
        return i, j, tuple(taps), r
    i, j = rng.integers(1, nx + 1, nobs).astype(np.int32), rng.integers(1, ny + 1, nobs).astype(np.int32)
    i[:4], j[:4] = [1, nx, 1, nx], [1, ny, ny, 1]
    i[6], j[6] = i[5], j[5]
    i, j, taps = csim.box_taps(nx, ny, i, j, 1, 1)
    return i, j, tuple(taps), r


def point_network(rng, grid, nobs):
    """point observations on distinct cells in a random order, so that no two rows share a value"""
    nx, ny = grid[0], grid[1]
    e = rng.permutation(nx * ny)[:nobs]
    return (e % nx + 1).astype(np.int32), (e // nx + 1).astype(np.int32), None, rng.uniform(0.5, 2.0, nobs)


def operator(X, t, i, j, taps):
    """h_k of the forecast members, (M, nobs), input order"""
    if taps is None:
        return X[obsnet.forecast(X.shape[0], t)][:, j, i]
    return obsop.h_members(X, t, i, j, taps)


def plan_order(csim, i, j, grid=GRID):
    """input indices in plan order, from the library's host-only plan and localisation table"""
    nx, ny, dx, dy, loc = grid
    table = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    lx, ly = (table.shape[1] - 1) // 2, (table.shape[0] - 1) // 2
    return etkf.plan_order(csim.ensemble_assim_plan(i, j, lx, ly)), (lx, ly)


def block_of(q):
    return np.asarray(q) // HELD_ROWS


def inactive_mask(rng, order):
    """about a tenth inactive; never none (but for a single observation, which stays active: a whole block else) and
    never a whole block of plan positions or of input indices; the row of the last plan position is active, so the
    last block is read by everything"""
    nobs = len(order)
    mask = (rng.uniform(size=nobs) >= 0.1).astype(np.uint8)
    pos = np.empty(nobs, dtype=np.int64)
    pos[order] = np.arange(nobs)               # plan position of every input index
    mask[order[nobs - 1]] = 1
    both = (block_of(pos), block_of(np.arange(nobs)))
    for blocks in both:
        for b in np.unique(blocks):
            if not mask[blocks == b].any():
                mask[np.flatnonzero(blocks == b)[0]] = 1
    if nobs > 1 and mask.all():
        # the first plan position that is not alone in a block
        mask[next(o for o in order[:-1] if all(np.count_nonzero(bl == bl[o]) > 1 for bl in both))] = 0
    return mask


Inputs = collections.namedtuple("Inputs", "case B t X0 X1 i j taps r slot mask y order pos H hb vb status gross")
Inputs.__doc__ = """B members with the truth at t (None: none), the states X0 and X1 that slot 0 and slot 1 are held from
(X1 is also the state at analysis time), the network, the slots, the mask, the values, the plan order and its inverse,
the held rows H (nobs, M) in input order, their (hb, vb), the status bytes under the background check TOL, and the
input indices of the gross errors"""

_inputs = {}


def inputs(csim, c):
    key = (c.M, c.nobs)
    if key in _inputs:
        return _inputs[key]
    M, nobs = c.M, c.nobs
    B = M if c.truth is None else M + 1
    t = truth_of(c.truth, B)
    X0, X1 = members(B, GRID, 40), members(B, GRID, 41)
    # the first draw of the network whose plan puts some observation into another 64-row block than its input index
    # is in (any draw, up to 64 rows), so that k_held_mv's scatter by idx shows
    for draw in range(16):
        rng = np.random.default_rng([31, M, nobs, draw])
        if c.kind == "point":
            i, j, taps, r = point_network(rng, GRID, nobs)
        else:
            i, j, taps, r = linear_network(csim, rng, GRID, c.kind, nobs)
        order, _ = plan_order(csim, i, j)
        pos = np.empty(nobs, dtype=np.int64)
        pos[order] = np.arange(nobs)
        if nobs <= HELD_ROWS or (block_of(pos) != block_of(np.arange(nobs))).any():
            break
    slot = rng.integers(0, 2, nobs)
    slot[:2] = [0, 1][:nobs]
    mask = inactive_mask(rng, order)
    H = held.assemble({0: X0, 1: X1}, slot, lambda S: operator(S, t, i, j, taps))
    hb, vb = held.row_mv(H)
    y = hb + 0.5 * np.sqrt(vb + r) * rng.standard_normal(nobs).clip(-2, 2)
    # two gross errors against the rows on active observations: the first active row of the second block of plan
    # positions where there is one (of 65 rows that is the tail's only row, so the last segment has nothing used; of
    # 128 and 129 the tail stays used), else the last active row; and the second active row of the first block.  A
    # single observation keeps its value, else nothing were used
    active = np.flatnonzero(mask == 1)
    by_pos = active[np.argsort(pos[active])]
    far = by_pos[pos[by_pos] >= HELD_ROWS]
    gross = [] if nobs == 1 else [int(far[0] if len(far) else by_pos[-1]), int(by_pos[1])]
    for n, o in enumerate(gross):
        y[o] = hb[o] + (50.0, -40.0)[n] * np.sqrt(vb[o] + r[o])
    status = screen.statuses(y, hb, vb, r, TOL, mask)
    _inputs[key] = Inputs(c, B, t, X0, X1, i, j, taps, r, slot, mask, y, order, pos, H, hb, vb, status, gross)
    return _inputs[key]


_weights = {}


def weights(csim, c, device):
    """(W, wbar) of the case's analysis: the restated Gram matrix over the used rows, then the library's host weights
    in the path's order; once per case and order"""
    key = (c.M, c.nobs, bool(device))
    if key not in _weights:
        x = inputs(csim, c)
        A = etkf.obs_gram(x.H.T, x.y, x.r, x.status == screen.USED, x.order)[0]
        w = csim.etkf_weights(A, INFLATION, order="round_robin" if device else "rows")
        _weights[key] = (w.W, w.wbar)
    return _weights[key]


# ---- wrong kernels ---------------------------------------------------------------------------------------------------

VARIANTS = ("last_block_untransformed", "block_from_block_0", "tail_outputs_as_last", "mv_at_plan_position",
            "row_rotated")


def excused(c):
    """variant -> reason, for the variants that a case cannot tell from the right kernel"""
    out = {}
    if c.nobs <= HELD_ROWS:
        out["block_from_block_0"] = "one block"
    if c.M % HELD_RB == 0:
        out["tail_outputs_as_last"] = "M % 4 = 0: no output tail"
    elif c.M % HELD_RB == 1:
        out["tail_outputs_as_last"] = "M % 4 = 1: the tail is output M - 1 alone"
    if c.nobs == 1:
        out["mv_at_plan_position"] = "one observation: plan position and input index are both 0"
    return out


def right_results(x, W, wbar):
    """(T, mean, variance): the transformed rows (nobs, M) and mv of the rows before, all in input order"""
    m, v = held.row_mv(x.H)
    return held.row_transform(x.H, W, wbar), m, v


def wrong_variants(x, W, wbar):
    """variant -> (T, mean, variance) in input order, as five wrong kernels would leave them.  The kernels see the rows
    in plan order, so the blocks are blocks of plan positions"""
    H, order, nobs, M = x.H, x.order, len(x.order), x.H.shape[1]
    Hp = H[order]                                  # row q: plan position q
    Tp = held.row_transform(Hp, W, wbar)
    mp, vp = held.row_mv(Hp)
    m, v = held.row_mv(H)
    blocks = -(-nobs // HELD_ROWS)

    def back(Ap):                                  # plan order -> input order
        out = np.empty_like(Ap)
        out[order] = Ap
        return out

    res = {}
    a = Tp.copy()
    a[(blocks - 1) * HELD_ROWS:] = Hp[(blocks - 1) * HELD_ROWS:]
    res["last_block_untransformed"] = (back(a), m, v)
    a = Tp.copy()
    for b in range(1, blocks):
        n = min(HELD_ROWS, nobs - b * HELD_ROWS)
        a[b * HELD_ROWS:b * HELD_ROWS + n] = Tp[:n]
    res["block_from_block_0"] = (back(a), m, v)
    a = Tp.copy()
    a[:, HELD_RB * (M // HELD_RB):] = Tp[:, M - 1:M]
    res["tail_outputs_as_last"] = (back(a), m, v)
    res["mv_at_plan_position"] = (back(Tp), mp, vp)   # out[2 q] in place of out[2 idx[q]]
    rot = np.roll(Hp, 1, axis=1)
    res["row_rotated"] = (back(held.row_transform(rot, W, wbar)),) + tuple(back(a) for a in held.row_mv(rot))
    return res


def differs(got, want):
    """some 64-bit pattern of (T, mean, variance) differs"""
    return any(not np.array_equal(np.asarray(g).view(np.int64), np.asarray(w).view(np.int64)) for g, w in zip(got, want))


# ---- the ROWS Gram matrix at the seams of the shared tile geometry -------------------------------------------------

# cols = M + 1 on both sides of the steps of tests/test_gpu_gram_share_seams.py: 1 -> 2 blocks a side (4, 5), and the
# block counts 253 -> 276 (88, 89), 496 -> 528 (124, 125), 990 -> 1035 (176, 177), 1035 -> 1081 (180, 181)
GRAM_COLS = [5, 88, 89, 124, 125, 177, 181]
GRAM_NOBS = [65, 129]
GRAM_BLOCKS = {5: 3, 88: 253, 89: 276, 124: 496, 125: 528, 177: 1035, 181: 1081}


def gram_blocks(cols):
    """gram_nblocks of csrc/gram_plan.hpp: 4 x 4 blocks of the upper triangle"""
    nblk = -(-cols // 4)
    return nblk * (nblk + 1) // 2


GramInputs = collections.namedtuple("GramInputs", "M X0 X1 X2 i j r slot mask y order H")

_gram_inputs = {}


def gram_inputs(csim, cols, nobs):
    """two slots held from X0 and X1, a third state X2 that is current when the matrix is formed"""
    key = (cols, nobs)
    if key not in _gram_inputs:
        M = cols - 1
        rng = np.random.default_rng([32, cols, nobs])
        X0, X1, X2 = (members(M, GRID, s) for s in (42, 43, 44))
        i, j, _, r = point_network(rng, GRID, nobs)
        order, _ = plan_order(csim, i, j)
        slot = rng.integers(0, 2, nobs)
        slot[:2] = [0, 1]
        mask = inactive_mask(rng, order)
        y = 3.0 + rng.standard_normal(nobs)
        H = held.assemble({0: X0, 1: X1}, slot, lambda S: operator(S, None, i, j, None))
        _gram_inputs[key] = GramInputs(M, X0, X1, X2, i, j, r, slot, mask, y, order, H)
    return _gram_inputs[key]
