"""tests/perturb_launch_cases.py — the cases of csim_ensemble_perturb's launch-seam test
(tests/test_gpu_ensemble_perturb_seams.py): a targeted list, a seeded fuzz and the far-tail constants.

`launch_choice` restates the tile height and the member shares that ens_launch_perturb (ensemble_perturb.hip) picks,
and `describe` what the kernel then does with a case: the LDS it asks for, its tiles, the parities of its Philox
pairs, where a periodic wrap falls.  Both are coverage aids for tests/test_ensemble_perturb_launch_host.py only; no
GPU assertion depends on them.  `fuzz_cases(seed, n)` is a pure function of its arguments."""
import numpy as np

import perturb_restatement as ref
from ensemble_fuzz_cases import SPACINGS

DEFAULT_SEED = 20261019
FUZZ_CASES = 60
MAX_RADIUS = 32  # CSIM_PERTURB_MAX_RADIUS
TX = 64          # cells per tile row

BC_CODE = {"d": 0, "n": 1, "p": 2}


def bc_codes(bc):
    return tuple(BC_CODE[k] for k in bc)


def launch_choice(nx, ny, M, centered, tile_rows=0, shares=0):
    """(TY, gridDim.y) of ens_launch_perturb for M forecast members and the two options (coverage aid only)"""
    tiles_x = -(-nx // TX)
    tiles32 = tiles_x * -(-ny // 32)
    want = 512 if centered else 2048
    tall = tile_rows == 32 if tile_rows else tiles32 * (1 if centered else M) >= want // 2
    tiles = tiles32 if tall else tiles_x * -(-ny // 8)
    if shares:
        s = min(shares, M)
    else:
        s = max(1, min(-(-want // tiles), M, 65535))
    return (32 if tall else 8), s


def make(B, t, nx, ny, bc, dx, dy, corr_len, centered, sigma, seed, draw, tile_rows=0, shares=0, name=None):
    """a case; `name` is its test id"""
    c = dict(B=B, t=t, nx=nx, ny=ny, bc=bc, dx=dx, dy=dy, corr_len=corr_len, centered=int(centered), sigma=sigma,
             seed=seed, draw=draw, tile_rows=tile_rows, shares=shares)
    c["name"] = name or (f"B{B}_t{t}_{nx}x{ny}_{bc}_c{corr_len:g}_cen{int(centered)}_ty{tile_rows}_s{shares}")
    return c


def forecast_members(c):
    return c["B"] - (c["t"] is not None)


def describe(c):
    """what the launch of case c reaches (coverage aid only)"""
    nx, ny, M = c["nx"], c["ny"], forecast_members(c)
    perx, pery = ref.axis_periodic(bc_codes(c["bc"]))
    rx, ry = ref.radius(c["dx"], c["corr_len"], nx, perx), ref.radius(c["dy"], c["corr_len"], ny, pery)
    TY, shares = launch_choice(nx, ny, M, c["centered"], c["tile_rows"], c["shares"])
    tiles_x, tiles_y = -(-nx // TX), -(-ny // TY)
    Px = nx if perx else nx + 2 * rx
    Py = ny if pery else ny + 2 * ry
    # the parity of the first slot of a lattice row of a tile, as perturb_field forms it
    parities, wrap_tiles_x = set(), []
    for tx in range(tiles_x):
        x0 = tx * TX
        tw = min(TX, nx - x0)
        col0 = (x0 - rx + nx) % nx if perx else x0
        parities |= {(b * Px + col0) & 1 for b in range(min(Py, 2))}
        if perx and (x0 - rx < 0 or x0 + tw + rx > nx):
            wrap_tiles_x.append(tx)
    wrap_tiles_y = [ty for ty in range(tiles_y)
                    if pery and (ty * TY - ry < 0 or ty * TY + min(TY, ny - ty * TY) + ry > ny)]
    t = c["t"]
    where = "absent" if t is None else "first" if t == 0 else "last" if t == c["B"] - 1 else "middle"
    return dict(M=M, rx=rx, ry=ry, TY=TY, shares=shares, centered=bool(c["centered"]),
                lds=8 * (TY + 2 * ry) * (2 * TX + 2 * rx),
                tiles_x=tiles_x, tiles_y=tiles_y, tiles=tiles_x * tiles_y,
                last_w=nx - (tiles_x - 1) * TX, last_h=ny - (tiles_y - 1) * TY,
                strided=M > shares, rem=M % shares,
                Px=Px, px_odd=bool(Px & 1), perx=perx, pery=pery,
                wrap_x=bool(wrap_tiles_x) and rx > 0, wrap_y=bool(wrap_tiles_y) and ry > 0,
                wrap_tiles_x=wrap_tiles_x if rx > 0 else [], wrap_tiles_y=wrap_tiles_y if ry > 0 else [],
                parities=parities, truth=where, auto=c["tile_rows"] == 0 and c["shares"] == 0)


def _seam_cases():
    S = []
    # ---- LDS: every instantiation above 64 KiB, both tall ones at the largest launch (R = 32 on both axes)
    for ty in (8, 32):
        for cen in (0, 1):
            S.append(make(3, None, 130, 67, "nnnn", 1.0, 1.0, 16.2, cen, 2.0, 8 + ty + cen, 1, tile_rows=ty,
                          name=f"lds_ty{ty}_cen{cen}"))
    # ---- the automatic seam, both options at 0: tiles32 = 3 * 3 = 9 for 130 x 67; 9 * 113 = 1017, 9 * 114 = 1026
    S.append(make(113, None, 130, 67, "dnpd", 1.0, 1.0, 1.0, 0, 0.5, 31, 0, name="auto_ty8_M113"))
    S.append(make(115, 57, 130, 67, "dnpd", 1.0, 1.0, 1.0, 0, 0.5, 31, 0, name="auto_ty32_M114"))
    # centered: 16 * 15 = 240 tiles of 32 rows, 16 * 16 = 256
    S.append(make(2, None, 1024, 480, "dddd", 1.0, 1.0, 1.0, 1, 1.0, 32, 0, name="auto_cen_ty8_240"))
    S.append(make(2, None, 1024, 512, "ddpp", 1.0, 1.0, 1.0, 1, 1.0, 33, 0, name="auto_cen_ty32_256"))
    # ---- tile edges: every ny around a tile height under both heights, every nx around a tile width
    nxs = [63, 64, 65, 128, 129]
    bcs = ["dddd", "pppp", "nndd", "ppnn", "ddpp", "npdn"]
    n = 0
    for ty in (8, 32):
        for ny in (7, 8, 9, 31, 32, 33):
            nx = nxs[n % 5]
            S.append(make(3 + n % 3, (None, 0, 2)[n % 3], nx, ny, bcs[n % 6], 1.0, 1.0, (0.0, 1.0, 2.0, 3.3)[n % 4],
                          n % 2, 0.75, 100 + n, n, tile_rows=ty, shares=(0, 2)[n % 2], name=f"edge_{nx}x{ny}_ty{ty}"))
            n += 1
    # ---- periodic wrap.  Periodic x, odd nx, three tiles at 32 rows: only the first and the last tile wrap, and every
    # pair after the wrap needs its second Philox call
    S.append(make(4, 1, 165, 40, "ppdd", 1.0, 1.0, 16.2, 0, 1.0, 41, 2, tile_rows=32, name="wrap_x_odd_ty32_R32"))
    S.append(make(4, None, 131, 33, "ppnn", 1.0, 1.0, 0.6, 1, 1.0, 42, 2, tile_rows=32, name="wrap_x_odd_ty32_R1"))
    # the periodic clip (n - 1) / 2 binds on both axes, odd and even n
    S.append(make(3, None, 33, 20, "pppp", 1.0, 1.0, 16.2, 0, 1.0, 43, 0, tile_rows=32, name="wrap_clip_33x20"))
    S.append(make(3, None, 65, 9, "pppp", 1.0, 1.0, 16.2, 1, 1.0, 44, 0, tile_rows=8, name="wrap_clip_65x9"))
    # periodic in y only, rows wrap across tiles of both heights
    S.append(make(3, 2, 70, 45, "ddpp", 1.0, 1.0, 5.0, 0, -1.0, 45, 0, tile_rows=8, name="wrap_y_only_ty8"))
    S.append(make(3, 0, 70, 45, "nnpp", 1.0, 1.0, 5.0, 1, 1.0, 46, 0, tile_rows=32, name="wrap_y_only_ty32"))
    # ---- anisotropy: R = 32 along one axis, 0 along the other
    for ty in (8, 32):
        S.append(make(3, None, 131, 40, "dddd", 1.0, 100.0, 16.2, ty == 8, 1.0, 51, 0, tile_rows=ty,
                      name=f"aniso_rx32_ry0_ty{ty}"))
        S.append(make(3, None, 70, 67, "nnnn", 100.0, 1.0, 16.2, ty == 32, 1.0, 52, 0, tile_rows=ty,
                      name=f"aniso_rx0_ry32_ty{ty}"))
    # ---- member shares
    S.append(make(65, None, 70, 20, "dnpd", 1.0, 1.0, 1.0, 0, 1.0, 61, 0, shares=1, name="shares_1_M65"))
    S.append(make(65, None, 70, 20, "dnpd", 1.0, 1.0, 1.0, 1, 1.0, 61, 0, tile_rows=32, shares=1,
                  name="shares_1_M65_cen"))
    S.append(make(12, None, 70, 40, "pppp", 1.0, 1.0, 2.0, 1, 1.0, 62, 0, tile_rows=32, shares=65535,
                  name="shares_M"))
    # shares < M, M % shares != 0, and the truth member in every place under that strided loop
    for t in (None, 0, 5, 10):
        for cen in (0, 1):
            S.append(make(11, t, 67, 35, "dnpd", 1.0, 0.8, 1.5, cen, 0.5, 63, 1, tile_rows=(8, 32)[cen], shares=3,
                          name=f"shares_3_t{t}_cen{cen}"))
    return S


SEAM_CASES = _seam_cases()

F_SET = [0.0, 0.4, 1.0, 2.5, 8.0, 16.2]
SIGMA_SET = [1.0, -1.0, 0.5, -0.7, 2.0]


def _pick(rng, values):
    return values[int(rng.integers(len(values)))]


def fuzz_cases(seed=DEFAULT_SEED, n=FUZZ_CASES):
    """corr_len = f min(dx, dy) with f <= 16.2 keeps every radius at or below 32: no case may be refused"""
    rng = np.random.default_rng(seed)
    cases = []
    for case in range(n):
        nx, ny, B = int(rng.integers(1, 201)), int(rng.integers(1, 101)), int(rng.integers(1, 41))
        bc = "".join(_pick(rng, "dnp") for _ in range(4))
        dx, dy = _pick(rng, SPACINGS)
        t = _pick(rng, [None, None, 0, B - 1, int(rng.integers(B))]) if B > 1 else None
        M = B - (t is not None)
        centered = int(rng.integers(2)) if M >= 2 else 0
        f = _pick(rng, F_SET)
        cases.append(make(B, t, nx, ny, bc, dx, dy, f * min(dx, dy), centered, _pick(rng, SIGMA_SET),
                          int(rng.integers(0, 1 << 64, dtype=np.uint64)), int(rng.integers(0, 1 << 32)),
                          tile_rows=_pick(rng, [0, 8, 32]), shares=_pick(rng, [0, 1, 2, 7, 65535]),
                          name=f"fuzz{case}"))
    return cases


def from_tuple(t):
    """a case of tests/test_gpu_ensemble_perturb.py's CASES"""
    return make(*t)


def start_state(c):
    """the members uploaded for case c: random interior and ghost ring, a negative zero in the interior"""
    rng = np.random.default_rng([c["B"], c["nx"], c["ny"], c["draw"]])
    X = rng.standard_normal((c["B"], c["ny"] + 2, c["nx"] + 2))
    X[:, 1, 1] = -0.0
    return X


# ---- the far tail of the normal quantile (r = sqrt(-ln t) > 5: t < exp(-25), 2.8e-11 per deviate) ---------------------
# A 64 x 64 "dddd" ensemble at dx = dy = 1 with corr_len 0 has taps [1], Px = 64 and p = w: the increment of a cell on a
# zero state with sigma = 1 is the deviate of lattice point row * 64 + col itself.  The seeds were found by a seed search
# on the CPU and checked with perturb_restatement.white; `value` is the restatement's deviate at that cell.
FAR_TAIL = [
    dict(seed=910914, draw=0, B=1, member=0, row=56, col=43, r=5.1315, value=-6.851148970055759),
    dict(seed=758713, draw=0, B=5, member=4, row=39, col=37, r=5.0527, value=6.735304553527277),
]
FAR_TAIL_N = 64


def far_tail_bits(ft):
    """the 64 bits normal_from_bits gets for the cell of a FAR_TAIL entry"""
    L = np.uint64(ft["row"] * FAR_TAIL_N + ft["col"])
    n = L >> np.uint64(1)
    o = ref.philox([n & ref.U32, n >> ref.S32, np.uint64(ft["member"]), np.uint64(ft["draw"])],
                   [ft["seed"] & 0xFFFFFFFF, ft["seed"] >> 32])
    s = int(L & np.uint64(1))
    return np.uint64(int(o[2 * s]) | (int(o[2 * s + 1]) << 32))
