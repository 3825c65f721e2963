"""numpy restatement of the 4D-ETKF block of include/csim.h (csim_obs_slots_present, csim_obs_network_hold,
csim_ensemble_assimilate_etkf_held), written from the text: which slots occur, the rows assembled from the states at
their slots' times, mv of a row and the transform of a row, which is espace_restatement's cell transform with the row
in the place of a cell's members.  tests/test_held_host.py pins it; tests/test_gpu_held.py uses it as the reference."""
import numpy as np

import espace_restatement as espace

MAX_SLOTS = 64


def slots_present(slot, nobs=None):
    """the mask of csim_obs_slots_present: bit s for every slot s that occurs; None: every observation in slot 0"""
    if slot is None:
        if nobs is not None and nobs < 1:
            raise ValueError("nobs must be >= 1")
        return 1
    slot = [int(s) for s in slot]
    if not slot:
        raise ValueError("nobs must be >= 1")
    mask = 0
    for s in slot:
        if not 0 <= s < MAX_SLOTS:
            raise ValueError("slot out of range")
        mask |= 1 << s
    return mask


def as_cells(H):
    """(nobs, M) rows as the interior cells of M members of a 1 x nobs grid, (M, 3, nobs + 2)"""
    H = np.asarray(H, dtype=np.float64)
    X = np.zeros((H.shape[1], 3, H.shape[0] + 2))
    X[:, 1, 1:-1] = H.T
    return X


def row_transform(H, W, wbar=None):
    """every row of H (nobs, M) as one cell's M members under csim_ensemble_transform(centered = 1)"""
    with np.errstate(all="ignore"):
        return espace.transform(as_cells(H), W, wbar, None, True)[:, 1, 1:-1].T.copy()


def row_mv(H):
    """(mean, variance) of every row, mv of csim_ensemble_relax: running sums from +0 in member order"""
    H = np.asarray(H, dtype=np.float64)
    n, M = H.shape
    with np.errstate(all="ignore"):
        s = np.zeros(n)
        for k in range(M):
            s = s + H[:, k]
        m = s / float(M)
        q = np.zeros(n)
        for k in range(M):
            d = H[:, k] - m
            q = q + d * d
        return m, q / (float(M) - 1.0)


def assemble(states, slot, operator):
    """H (nobs, M): row o is operator(states[slot[o]])[:, o], the (M, nobs) operator values of the state that was
    current when slot[o] was held"""
    slot = np.asarray(slot)
    per = {int(s): operator(states[int(s)]) for s in np.unique(slot)}
    return np.stack([per[int(slot[o])][:, o] for o in range(len(slot))])


# ---- the claim of the 4D filter: a hold, a run and a held analysis against an analysis and the same run ---------------
#
# The model is affine in the state (one common physics), and transform(centered = 1) replaces every member by an affine
# combination of the members whose coefficients sum to one, so the two orders agree up to rounding.

CLAIM_GRID = (37, 21, 1.0, 1.0, 2.5)
CLAIM_NOBS = 40
CLAIM_PHYSICS = (0.05, 0.4, 1.0, 0.5)   # D, dt, vx, vy: 0.4 cells a step along x, 0.2 along y
CLAIM_STEPS = 10
CLAIM_VALUE = 0.5                       # of the Dirichlet sides
CLAIM_KINDS = ("point", "bilinear", "box")


def claim_scenarios():
    """the 32 seeded scenarios: (seed, kind, M, inflation, bcs).  No periodic side: a periodic ghost is part of the state
    at the first step of a run, and a transform leaves the ghost ring alone"""
    return [(s, CLAIM_KINDS[s % 3], (5, 8, 12, 33)[s % 4], (1.0, 1.1)[(s // 2) % 2], ("dddd", "dnnd")[(s // 4) % 2])
            for s in range(32)]


def claim_case(csim, scenario):
    """the members (B = M + 1, the last one the truth), the network and the values of a scenario"""
    seed, kind, M, lam, bcs = scenario
    nx, ny = CLAIM_GRID[0], CLAIM_GRID[1]
    rng = np.random.default_rng([77, seed])
    # smooth fields, so that ten steps of advection move something that an observation sees
    jj, ii = np.meshgrid(np.arange(ny + 2), np.arange(nx + 2), indexing="ij")
    X = np.empty((M + 1, ny + 2, nx + 2))
    for k in range(M + 1):
        a, b, c, d = rng.uniform(0.5, 1.5), rng.uniform(0, 2 * np.pi), rng.uniform(0.5, 1.5), rng.uniform(0, 2 * np.pi)
        X[k] = 3.0 + a * np.sin(2 * np.pi * ii / 12.0 + b) * np.cos(2 * np.pi * jj / 9.0 + d) + 0.3 * c * np.sin(
            2 * np.pi * (ii + jj) / 7.0 + b + d)
    r = rng.uniform(0.05, 0.2, CLAIM_NOBS)
    if kind == "bilinear":
        i, j, taps = csim.bilinear_taps(nx, ny, rng.uniform(1, nx, CLAIM_NOBS), rng.uniform(1, ny, CLAIM_NOBS))
        taps = tuple(taps)
    else:
        i = rng.integers(1, nx + 1, CLAIM_NOBS).astype(np.int32)
        j = rng.integers(1, ny + 1, CLAIM_NOBS).astype(np.int32)
        taps = None
        if kind == "box":
            i, j, taps = csim.box_taps(nx, ny, i, j, 1, 1)
            taps = tuple(taps)
    z = rng.standard_normal(CLAIM_NOBS)
    return X, i, j, taps, r, z


def claim_cpu(csim, ora, etkf, operator, scenario):
    """the two paths and the analysis with rows from the wrong time, in numpy with the oracle's stepping and the
    restatements.  Returns (X2 of the held path, X2 of the analysis-first path, X2 of the plain analysis at the end,
    the forecast X2 without any analysis); the truth member is the last one and the values are its operator values at
    t1 plus sqrt(r) z"""
    seed, kind, M, lam, bcs = scenario
    nx, ny, dx, dy, loc = CLAIM_GRID
    D, dt, vx, vy = CLAIM_PHYSICS
    X1, i, j, taps, r, z = claim_case(csim, scenario)
    t = M
    table = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    lx, ly = (table.shape[1] - 1) // 2, (table.shape[0] - 1) // 2
    order = etkf.plan_order(csim.ensemble_assim_plan(i, j, lx, ly))
    bc = ora.bc_codes(bcs)

    def run(X):
        out = X.copy()
        for k in range(out.shape[0]):
            u = np.ascontiguousarray(out[k])
            ora.run_single(u, dx, dy, D, vx, vy, dt, bc, CLAIM_STEPS, CLAIM_VALUE)
            out[k] = u
        return out

    def weights(X, y):
        A = etkf.obs_gram(operator(X, t, i, j, taps), y, r, True, order)[0]
        return etkf.etkf_weights(A, lam, csim.sym_eigen)[:2]

    truth = operator(X1, None, i, j, taps)[t]
    y = truth + np.sqrt(r) * z
    W, wbar = weights(X1, y)
    X2 = run(X1)
    held_path = espace.transform(X2, W, wbar, t, True)
    first_path = run(espace.transform(X1, W, wbar, t, True))
    W2, wbar2 = weights(X2, y)
    wrong = espace.transform(X2, W2, wbar2, t, True)
    return held_path, first_path, wrong, X2


def claim_error(a, b, forecast, M):
    """the largest difference of the forecast members' interiors, relative to the RMS analysis increment b - forecast"""
    inc = (b - forecast)[:M, 1:-1, 1:-1]
    return float(np.abs((a - b)[:M, 1:-1, 1:-1]).max() / np.sqrt(np.mean(inc * inc)))
