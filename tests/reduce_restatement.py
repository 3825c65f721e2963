"""The reductions of include/csim.h (csim_field_minmax / _sum / _linf_diff, csim_stepper_minmax / _sum,
csim_ensemble_minmax / _sum) restated in numpy, their references, and the cases the host and the GPU tests share.

The sum's order (k_reduce<1> of kernels.hip, for one field or one member per blockIdx.y, and fold_partials of api.cpp),
every + one IEEE fp64 addition:
  * the window has `rows` rows; G = min(rows, cap) blocks, cap = 1024 (REDUCE_BLOCKS: Field, Stepper) or 64
    (ENS_REDUCE_ROWS: ensemble); block b takes rows b, b + G, b + 2 G, ... in that order;
  * lane t of the block's 256 adds columns t, t + 256, ... of each of its rows, serially from +0.0;
  * in each of the four 64-lane waves an xor butterfly with masks 32, 16, 8, 4, 2, 1: v = v + v[lane ^ m];
  * lane 0 of waves 0, 1, 2, 3 are added in that order: the block's partial;
  * the host adds the partials of blocks 0, 1, ..., G - 1 in that order, starting from partial 0.
Arrays are in the reference layout, (ny + 2, nx + 2) with the ghost ring; sum and linf span the interior, minmax the
whole array."""
import math

import numpy as np

CAP_FIELD, CAP_ENSEMBLE, LANES = 1024, 64, 256

# (nx, ny) of the Field / Stepper cases: widths below, on and past one trip of the column loop, one row, one column,
# ny + 2 == 1024, the second trip of the row loop for minmax (ny + 2 = 1025) and for sum / linf (ny = 1025), three
# ragged trips
SHAPES = [(1, 1), (1, 300), (300, 1), (255, 3), (256, 3), (257, 3), (513, 62), (130, 1022), (130, 1023), (130, 1024),
          (130, 1025), (67, 2051)]
ENS_SHAPES = [(nx, ny) for nx in (1, 257) for ny in (1, 62, 63, 64, 65, 129)]
ENS_MEMBERS = [1, 3]


def trips(rows, cap):
    """trips of the row loop of the block with the most rows"""
    return -(-rows // min(rows, cap))


def block_partials(x, cap, keep=None):
    """the per-block partial sums of the window x (rows, cols); keep: boolean mask of the cells that are added"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    rows, cols = x.shape
    G = min(rows, cap)
    acc = np.zeros((G, LANES))
    with np.errstate(all="ignore"):
        for r0 in range(0, rows, G):  # one trip of every block's row loop
            n = min(G, rows - r0)
            for c0 in range(0, cols, LANES):  # one trip of every lane's column loop
                w = min(LANES, cols - c0)
                new = acc[:n, :w] + x[r0:r0 + n, c0:c0 + w]
                acc[:n, :w] = new if keep is None else np.where(keep[r0:r0 + n, c0:c0 + w], new, acc[:n, :w])
        v = acc.reshape(G, 4, 64)
        lane = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lane ^ m]
        p = v[:, 0, 0]
        for w in (1, 2, 3):
            p = p + v[:, w, 0]
    return p


def merge(partials, skip=None):
    """the host's finish: the partials added in block order (skip: one block left out)"""
    r = None
    with np.errstate(all="ignore"):
        for k, p in enumerate(partials):
            if k == skip:
                continue
            r = np.float64(p) if r is None else r + np.float64(p)
    return float(r)


def restated_sum(u, cap=CAP_FIELD):
    """csim_field_sum / csim_stepper_sum (cap 1024) or one member of csim_ensemble_sum (cap 64) of the array u"""
    return merge(block_partials(u[1:-1, 1:-1], cap))


# ---- references ------------------------------------------------------------------------------------------------

def ref_sum(u):
    """the interior's sum, correctly rounded (inf / nan as IEEE addition gives them)"""
    x = u[1:-1, 1:-1].ravel()
    if not np.isfinite(x).all():
        with np.errstate(all="ignore"):
            return float(np.sum(np.where(np.isfinite(x), 0.0, x)))
    return math.fsum(x.tolist())


def ref_linf(a, b):
    """max |a - b| over the interior; numpy's max propagates NaN"""
    with np.errstate(all="ignore"):
        return float(np.abs(a - b)[1:-1, 1:-1].max())


def ref_minmax(u):
    """the reference's std::min_element / max_element over the whole array (ora_minmax of oracle/cpu_stepper.c)"""
    import ctypes as C

    from oracle import cpu_oracle as ora
    a = np.ascontiguousarray(u, dtype=np.float64)
    out = (C.c_double * 2)()
    ora.lib().ora_minmax(a.ctypes.data_as(C.POINTER(C.c_double)), a.size, out)
    return out[0], out[1]


def sum_additions(nx, ny, cap):
    """k of the bound: the most additions one value passes through — the lane's serial adds (column trips times row
    trips), 6 butterfly steps, 3 wave adds, G - 1 host adds"""
    G = min(ny, cap)
    return -(-nx // LANES) * -(-ny // G) + 6 + 3 + (G - 1)


def sum_bound(u, cap=CAP_FIELD):
    """gamma_k sum |x|, gamma_k = k u / (1 - k u), u = 2^-53: the classic bound of any summation order in which no
    value goes through more than k additions (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., 4.2)"""
    ny, nx = u.shape[0] - 2, u.shape[1] - 2
    k = sum_additions(nx, ny, cap)
    ku = k * 2.0 ** -53
    return ku / (1.0 - ku) * math.fsum(np.abs(u[1:-1, 1:-1]).ravel().tolist())


# ---- cases -----------------------------------------------------------------------------------------------------

def field(nx, ny, seed=0):
    """Gaussian noise on the whole array: the ghost ring is non-zero too, and larger than the interior's values, so a
    sum or an L-inf that let a ghost in would show"""
    rng = np.random.default_rng([seed, nx, ny])
    u = rng.standard_normal((ny + 2, nx + 2))
    ring = np.ones_like(u, dtype=bool)
    ring[1:-1, 1:-1] = False
    u[ring] = u[ring] * 3.0 + np.where(u[ring] < 0, -5.0, 5.0)
    return u


def positions(nx, ny, cap=CAP_FIELD):
    """{label: (j, i)} array positions (row, column of the (ny + 2, nx + 2) array) where extrema, differences and
    non-finite values are planted: the ghost corners and a mid-point of each ghost line, interior columns 255 / 256 /
    257 (the seam between two trips of the column loop, for windows starting at column 0 and at column 1), the last
    interior row, and the first row of every further trip of the row loop — of the whole-array window (minmax) and of
    the interior window (sum, linf)"""
    jm, im = (ny + 1) // 2, (nx + 1) // 2
    pos = {"corner_bl": (0, 0), "corner_br": (0, nx + 1), "corner_tl": (ny + 1, 0), "corner_tr": (ny + 1, nx + 1),
           "ghost_bottom": (0, im), "ghost_top": (ny + 1, im), "ghost_left": (jm, 0), "ghost_right": (jm, nx + 1),
           "first": (1, 1), "last_row": (ny, im)}
    for i in (255, 256, 257):
        if i <= nx:
            pos[f"col{i}"] = (jm, i)
    G = min(ny + 2, cap)
    for k in range(1, trips(ny + 2, cap)):  # whole-array window: rows k G
        pos[f"whole_trip{k}"] = (k * G, im)
    G = min(ny, cap)
    for k in range(1, trips(ny, cap)):  # interior window: rows 1 + k G
        pos[f"interior_trip{k}"] = (1 + k * G, im)
    return pos


def is_interior(p, nx, ny):
    return 1 <= p[0] <= ny and 1 <= p[1] <= nx


def lane_seats(nx, ny):
    """interior positions read by lane 0 of a block's first wave and by the last lane of its last wave that has a
    cell: (1, 1) and, in the last interior row, the column of lane min(nx, 256) - 1 (lane 63 of wave 3 where
    nx >= 256, the last lane that has a cell in narrower fields)"""
    return {"lane0": (1, 1), "lane_last": (ny, min(nx, LANES))}
