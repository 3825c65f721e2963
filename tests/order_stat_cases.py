"""tests/order_stat_cases.py — the cases of the order-statistic seam test (tests/test_gpu_order_stat_seams.py) for
csim_ensemble_quantiles* and csim_ensemble_verify*: member counts, 0/1 and structured inputs, levels that read every
sorted position, and grid shapes that put the dense layout on a row seam.  numpy only.

`sort_form`, `sort_tile` and `loader_trips` restate for_sort_form, sort_tile and CSIM_LOAD_TILE of
csrc/ensemble_cell.hpp; MEMBER_SEAMS is built from them, not typed in.  What the lists reach is checked on the CPU by
tests/test_order_stat_cases_host.py.  A count in MEMBER_SEAMS is the number B of members of the ensemble: the
quantiles sort all B, the verification sorts M = B forecast members against a host truth and M = B - 1 against a truth
member.

Inputs come as columns, an array (B, n) with one cell's members per column; `pack` lays columns out on the smallest
grid of PACK_ROW dense cells per row that holds them."""
import numpy as np

DEFAULT_SEED = 20261020

SORT_LDS_BUDGET = 64 * 1024   # ensemble_cell.hpp
SORT_TILE_MAX = 16
SORT_MAX_VALUES = 4096        # QUANT_MAX_MEMBERS = VERIFY_MAX_MEMBERS
MAX_LEVELS = 16               # QUANT_MAX_LEVELS
VERIFY_GRID_MAX = 1024        # workgroups of a verification launch, at most
VERIFY_LANE_CELLS = 256       # cells per workgroup of the verification's lane form

LANE_P = (1, 2, 4, 8, 16, 32, 64)
WAVE_E = (2, 4, 8, 16, 32, 64)


# ---- the restatements ----------------------------------------------------------------------------------------------

def sort_form(n):
    """("lane", P) or ("wave", E) of for_sort_form for n values"""
    assert 1 <= n <= SORT_MAX_VALUES
    for P in LANE_P:
        if n <= P:
            return "lane", P
    for E in WAVE_E:
        if n <= 64 * E:
            return "wave", E


def sort_tile(members, extra=0):
    """(ct, stride, lds bytes) of sort_tile: the tile of `members` members with `extra` bytes kept behind it"""
    stride = members | 1
    ct = SORT_TILE_MAX
    while ct > 4 and ct * stride * 8 + extra > SORT_LDS_BUDGET:
        ct >>= 1
    return ct, stride, ct * stride * 8 + extra


KINDS = ("quantiles", "verify_truth", "verify_member")


def forecast(kind, B):
    """the number of values sorted per cell of an ensemble of B members"""
    return B - (kind == "verify_member")


def tile_of(kind, B):
    """the wave form's tile for an ensemble of B members: the quantiles keep nothing behind it, the verification the
    M + 1 bins of its rank histogram (M = B with a host truth, B - 1 with a truth member; the tile holds all B)"""
    return sort_tile(B, 0 if kind == "quantiles" else 4 * (forecast(kind, B) + 1))


def ct_switches(kind):
    """every B with a wave form at B and B + 1 whose tiles differ in ct, as (B, B + 1)"""
    return [(B, B + 1) for B in range(66, SORT_MAX_VALUES)
            if sort_form(forecast(kind, B))[0] == "wave" and tile_of(kind, B)[0] != tile_of(kind, B + 1)[0]]


def loader_trips(members, step, m0):
    """trips of CSIM_LOAD_TILE's eight-deep loop for a thread whose first member is m0 < step = 256 / ct"""
    return max(0, -(-(members - m0 - 7 * step) // (8 * step)))


def loader_changes(step, lo=65, hi=2049):
    """the counts B in lo..hi that the quantiles load with this step and at which the first (m0 = 0) or the last
    (m0 = step - 1) thread makes one more eight-deep trip than at B - 1"""
    ct = 256 // step
    sig = lambda B: (loader_trips(B, step, 0), loader_trips(B, step, step - 1))  # noqa: E731
    return [B for B in range(lo + 1, hi + 1)
            if tile_of("quantiles", B)[0] == ct == tile_of("quantiles", B - 1)[0] and sig(B) != sig(B - 1)]


def loader_seams():
    """per step: the first thread's first trip within the step's range, the count at which every thread has made it
    (one more starts the tail loop), and the first thread's next trip.  Above 1024 members, where uploads grow, only the
    last such pair below 2048 and 2048 itself."""
    out = []
    for step in (16, 32, 64):
        ch = loader_changes(step)
        for B in (ch[:3] if step < 64 else ch[-2:]):
            out += [B - 1, B]
            if loader_trips(B, step, step - 1) != loader_trips(B - 1, step, step - 1):
                out.append(B + 1)
    return out


def _member_seams():
    S = set()
    for P in LANE_P:                       # the smallest count, the full network, one more
        S |= {P // 2 + 1, P, P + 1}
    for E in WAVE_E:
        S |= {32 * E + 1, 64 * E, 64 * E + 1}
    for kind in KINDS:                     # both sides of every ct switch, +-2
        for lo, hi in ct_switches(kind):
            S |= set(range(lo - 2, hi + 3))
    S |= set(loader_seams())
    S |= {2047, 2048, 2049, 3072, 4095, 4096}
    return sorted(B for B in S if 1 <= B <= SORT_MAX_VALUES)


MEMBER_SEAMS = _member_seams()

# ensembles whose truth member is put on a lane boundary of a full wave network of the other B - 1 members
TRUTH_LANE_MEMBERS = [513, 1025, 4097]


# ---- inputs --------------------------------------------------------------------------------------------------------

PACK_ROW = 37          # dense cells per row of a packed grid: odd, no multiple of a tile or of a wave
CELL_CAP = 4096        # cells of a packed grid at most: 4096 members x 4096 cells x 8 bytes = 134 MB < 150 MB


def pack(cols):
    """columns (B, n) -> members (B, ny + 2, nx + 2) on the smallest grid of PACK_ROW cells per row (three rows at
    least) that holds them; the cells left over repeat the columns from the first"""
    B, n = cols.shape
    rows = max(3, -(-n // PACK_ROW))
    cells = rows * PACK_ROW
    assert cells <= CELL_CAP, f"{cells} cells: more than the upload cap of {CELL_CAP}"
    return np.ascontiguousarray(cols[:, np.arange(cells) % n]).reshape(B, rows, PACK_ROW)


def zero_one_exhaustive(M):
    """(M, ny + 2, nx + 2): dense cell c holds the 0/1 pattern c mod 2^M, member m its bit m; the first 2^M cells are
    every pattern (the 0-1 principle: a network that sorts these sorts everything)"""
    assert 1 <= M <= 16
    nx2, ny2 = max(3, 1 << -(-M // 2)), max(3, 1 << (M // 2))
    c = (np.arange(ny2 * nx2) % (1 << M)).reshape(ny2, nx2)
    return np.array([(c >> m) & 1 for m in range(M)], dtype=np.float64)


def zero_one_count_list(M):
    """the counts of ones of zero_one_counts: every j = 0..M, or above 1024 members 0, 1, M - 1, M and every multiple
    of 64 with its two neighbours"""
    if M <= 1024:
        return list(range(M + 1))
    js = {0, 1, M - 1, M}
    for j in range(64, M, 64):
        js |= {j - 1, j, j + 1}
    return sorted(j for j in js if 0 <= j <= M)


def zero_one_counts(M, reps, seed=DEFAULT_SEED):
    """columns (M, n): every count of ones of zero_one_count_list(M), each at `reps` random placements"""
    rng = np.random.default_rng([seed, M, 1])
    js = np.repeat(zero_one_count_list(M), reps)
    cols = (np.arange(M)[:, None] < js[None, :]).astype(np.float64)
    return rng.permuted(cols, axis=0)


def bit_reversed(M):
    """0..M-1 ordered by their bit-reversed value over ceil(log2 M) bits"""
    bits = max(1, (M - 1).bit_length())
    return np.array(sorted(range(M), key=lambda k: int(format(k, f"0{bits}b")[::-1], 2)), dtype=np.int64)


def structured(M, seed=DEFAULT_SEED):
    """(columns (M, n), names, n_distinct): one pattern per column.  The first n_distinct columns hold M distinct
    finite values each (ascending, descending, rotations of the sorted sequence by every multiple of 64 and one either
    side of it, organ pipe, bit-reversed order); then come the patterns with ties, a +0 / -0 mix, and real +inf
    members that must coexist with the network's +inf pads."""
    rng = np.random.default_rng([seed, M, 2])
    asc = np.sort(rng.standard_normal(M))
    while len(np.unique(asc)) < M:   # (never, in practice)
        asc = np.sort(rng.standard_normal(M))
    pats = [("ascending", asc), ("descending", asc[::-1])]
    for r in range(64, M, 64):
        for s in (r - 1, r, r + 1):
            if 0 < s < M:
                pats.append((f"rotated by {s}", np.roll(asc, s)))
    pats.append(("organ pipe", np.concatenate([asc[0::2], asc[1::2][::-1]])))
    pats.append(("bit-reversed", asc[bit_reversed(M)]))
    n_distinct = len(pats)
    k = np.arange(M)
    pats.append(("all equal", np.full(M, 0.25)))
    pats.append(("two alternating", np.where(k & 1, 1.5, -0.5)))
    pats.append(("three values", rng.choice([-1.0, 0.0, 1.0], M)))
    pats.append(("signed zeros", np.where(rng.random(M) < 0.5, 0.0, -0.0)))
    pats.append(("zeros among values", np.where(k % 3 == 0, 0.0, np.where(k % 3 == 1, -0.0, asc))))
    top = asc.copy()
    top[: max(1, M // 3)] = np.inf
    pats.append(("a third +inf, first", top))
    pats.append(("every third +inf", np.where(k % 3 == 2, np.inf, asc[::-1])))
    pats.append(("all but one +inf", np.where(k == M // 2, -1.0, np.inf)))
    return np.array([p for _, p in pats]).T.copy(), [n for n, _ in pats], n_distinct


def all_positions_levels(M):
    """the levels k / (M - 1), k = 0..M-1, in calls of at most MAX_LEVELS: between them they read every sorted value"""
    qs = [0.0] if M == 1 else [k / (M - 1) for k in range(M)]
    return [qs[i:i + MAX_LEVELS] for i in range(0, M, MAX_LEVELS)]


def sorted_quantiles(a, qs):
    """np.quantile(a, qs, axis=0) from one np.sort: numpy's "linear" method spelled out (virtual index (B - 1) q, its
    floor and the next index, numpy's two-sided interpolation, NaN where a member is NaN).  np.quantile partitions
    around every level, which for thousands of levels takes seconds; the CPU test holds this to np.quantile bit for
    bit"""
    B = a.shape[0]
    with np.errstate(all="ignore"):
        s = np.sort(a, axis=0)
        nan = np.isnan(s[-1])
        out = np.empty((len(qs),) + a.shape[1:])
        for n, q in enumerate(qs):
            v = float(B - 1) * q
            lo = int(np.floor(v))
            lo, hi, g = (B - 1, B - 1, v + 1) if v >= B - 1 else (lo, lo + 1, v - lo)
            d = s[hi] - s[lo]
            out[n] = np.where(nan, np.nan, s[hi] - d * (1 - g) if g >= 0.5 else s[lo] + d * g)
    return out


# ---- layout --------------------------------------------------------------------------------------------------------

def _layout_shapes():
    """(nx, ny): rows of 63 .. 129 dense cells, with the ny + 2 at which the cell count is a multiple of 256 (so also
    of 64 and of every tile) and one row more and fewer; then a grid whose 64-cell groups span 21 rows, and a single
    interior row"""
    S = []
    for nx2 in (63, 64, 65, 127, 128, 129):
        ny2 = 256 // np.gcd(nx2, 256)
        while ny2 < 4:
            ny2 *= 2
        S += [(nx2 - 2, int(ny2) - 2 + d) for d in (-1, 0, 1)]
    return S + [(1, 300), (1000, 1)]


LAYOUT_SHAPES = _layout_shapes()

# the verification's lane form launches exactly VERIFY_GRID_MAX workgroups for the first, and needs one more for the
# second: only its workgroup 0 loops
GRID_MAX_SHAPES = [(510, 510), (598, 435)]
