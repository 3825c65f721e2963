"""numpy restatements of the ensemble-space block of include/csim.h: the Gram matrix in its stated order, projection,
transform, and the composition behind csim_ensemble_eofs; an exact reference of the Gram matrix and its derived bound;
and the case lists that tests/test_espace_host.py and tests/test_gpu_espace.py share.

Every restatement does one rounded numpy operation per operation of the definition (numpy never contracts a * b + c),
so the GPU result can be compared bit for bit."""
import math
from fractions import Fraction

import numpy as np

SEG = 64
MAX_MEMBERS = 256
U = 2.0 ** -53


def forecast(B, t):
    """indices of the forecast members of B members without the truth member t (None: all)"""
    return [k for k in range(B) if k != t]


def gram_plan(M, nx, ny):
    """(nseg, Gc) of csim_ensemble_gram_plan"""
    nseg = -(-nx * ny // SEG)
    cap = 1024 if M <= 64 else 256 if M <= 128 else 64
    return nseg, min(nseg, cap)


def perturbations(X, t, centered):
    """(p, m): p_k of every cell of the (B, ny+2, nx+2) array X for the forecast members in order, and the mean (None
    when not centered)"""
    x = X[forecast(X.shape[0], t)]
    if not centered:
        return x.copy(), None
    s = np.zeros(x.shape[1:])
    for k in range(x.shape[0]):
        s = s + x[k]
    m = s / float(x.shape[0])
    return x - m, m


def interior_rows(p):
    """(M, nx ny): the interior of every member, cell e = (j - 1) nx + (i - 1)"""
    return np.ascontiguousarray(p[:, 1:-1, 1:-1]).reshape(p.shape[0], -1)


def gram(X, t=None, centered=True):
    """G of csim_ensemble_gram: vectorised over the classes and the M x M block, a loop over trips x 64 cells"""
    p, _ = perturbations(X, t, centered)
    P = interior_rows(p)
    M, cells = P.shape
    ny, nx = X.shape[1] - 2, X.shape[2] - 2
    nseg, Gc = gram_plan(M, nx, ny)
    acc = np.zeros((Gc, M, M))
    # the classes are independent: a few at a time, so that their sums stay in cache through the cell loop
    few = max(1, (1 << 18) // (M * M))
    term = np.empty((min(few, Gc), M, M))
    for g0 in range(0, Gc, few):
        g1 = min(Gc, g0 + few)
        for trip in range(-(-nseg // Gc)):
            for c in range(SEG):
                # classes g = g0 .. g0 + n - 1 have a cell c in this trip: e = (g + trip Gc) 64 + c increases with g
                first = (trip * Gc + g0) * SEG + c
                if first >= cells:
                    break
                n = min(g1 - g0, (cells - 1 - first) // SEG + 1)
                v = P[:, first:first + n * SEG:SEG].T  # (n, M)
                np.multiply(v[:, :, None], v[:, None, :], out=term[:n])
                np.add(acc[g0:g0 + n], term[:n], out=acc[g0:g0 + n])
    G = acc[0]
    for g in range(1, Gc):
        G = G + acc[g]
    return G


def class_cells(M, nx, ny):
    """the most cells that one class sums"""
    cells = nx * ny
    nseg, Gc = gram_plan(M, nx, ny)
    most = 0
    for g in range(Gc):
        n = sum(min(SEG, cells - q * SEG) for q in range(g, nseg, Gc))
        most = max(most, n)
    return most


def gram_exact(P):
    """the exact Gram matrix of the rows of P (M, cells) as Fractions"""
    M = P.shape[0]
    F = [[Fraction(float(v)) for v in row] for row in P]
    return [[sum((F[a][c] * F[b][c] for c in range(P.shape[1])), Fraction(0)) for b in range(M)] for a in range(M)]


def gram_bound(P, nx, ny):
    """gamma_k sum |p_a p_b| per entry, gamma_k = k u / (1 - k u): every product is rounded once, then goes through at
    most (cells of its class) additions of the class's running sum and Gc - 1 of the fold, so no term meets more than
    k = 1 + most cells of one class + (Gc - 1) roundings (Higham, Accuracy and Stability, 2nd ed., 4.2; the argument of
    sum_bound in tests/reduce_restatement.py).  Derived, not tuned."""
    M = P.shape[0]
    _, Gc = gram_plan(M, nx, ny)
    k = 1 + class_cells(M, nx, ny) + (Gc - 1)
    ku = k * U
    A = np.abs(P)
    return ku / (1.0 - ku) * np.array([[math.fsum((A[a] * A[b]).tolist()) for b in range(M)] for a in range(M)])


def project(X, W, t=None, centered=True):
    """(K, ny+2, nx+2) of csim_ensemble_project"""
    p, _ = perturbations(X, t, centered)
    W = np.asarray(W, dtype=np.float64).reshape(p.shape[0], -1)
    s = np.zeros((W.shape[1],) + p.shape[1:])
    for k in range(p.shape[0]):
        s = s + p[k][None] * W[k][:, None, None]
    return s


def transform(X, W, wbar=None, t=None, centered=True):
    """the members after csim_ensemble_transform: the interior of the forecast members replaced, every other bit kept"""
    p, m = perturbations(X, t, centered)
    s = project(X, W, t, centered)
    if centered:
        mp = m
        if wbar is not None:
            d = np.zeros(m.shape)
            for k in range(p.shape[0]):
                d = d + p[k] * float(wbar[k])
            mp = m + d
        s = mp + s
    out = X.copy()
    for r, k in enumerate(forecast(X.shape[0], t)):
        out[k, 1:-1, 1:-1] = s[r, 1:-1, 1:-1]
    return out


def eofs_weights(G, n_modes, sym_eigen):
    """(lambda, pcs, W, null) of csim_ensemble_eofs from the centered Gram matrix G and the library's sym_eigen"""
    M = G.shape[0]
    e = sym_eigen(G)
    lam, V = e.lambda_, e.V
    floor = (float(M) * 2.0 ** -52) * lam[0]
    K = n_modes
    null = np.array([bool(lam[r] <= floor or lam[r] <= 0.0) for r in range(K)])
    W, pcs = np.zeros((M, K)), np.zeros((M, K))
    for r in range(K):
        if not null[r]:
            root = np.sqrt(lam[r])
            W[:, r] = V[:, r] / root
            pcs[:, r] = V[:, r] * root
    return lam[:K].copy(), pcs, W, null


# ---- cases -----------------------------------------------------------------------------------------------------------

def members(B, nx, ny, seed=0, offset=3.0):
    """B random members on the whole array, ghost ring included, around a mean field that is far from zero, so that a
    result that forgot to centre, or centred with another mean, differs in every bit"""
    rng = np.random.default_rng([seed, B, nx, ny])
    base = offset + rng.standard_normal((ny + 2, nx + 2))
    return base[None] + 0.5 * rng.standard_normal((B, ny + 2, nx + 2))


def truth_of(kind, B):
    return {"none": None, "first": 0, "middle": B // 2, "last": B - 1}[kind]


# (nx, ny, M, truth kind, centered): every shape, every M and every truth position of the list appears
GRAM_SMALL = [
    (1, 1, 1, "none", 1), (1, 1, 2, "first", 0), (7, 9, 3, "middle", 1), (7, 9, 12, "last", 0),
    (8, 8, 2, "last", 1), (8, 8, 63, "none", 1), (5, 13, 64, "first", 1), (5, 13, 3, "none", 0),
    (130, 67, 12, "middle", 1), (130, 67, 64, "last", 0), (1, 300, 63, "middle", 0), (1, 300, 1, "first", 1),
]
# seams of the class loop: nseg = cap, cap + 1, three ragged trips; the caps of 65 .. 128 and 129 .. 256 members
GRAM_SEAMS = [
    (64, 1024, 3), (64, 1025, 3), (64, 2049, 3),
    (64, 256, 65), (64, 257, 65), (64, 256, 128), (64, 257, 128),
    (64, 64, 129), (64, 65, 129), (64, 64, 256), (64, 65, 256),
]
# and a class that carries its sums from a full segment into a ragged last one, of 2, 1 and 1 cells: the staged rows
# past the last cell are then the previous segment's, and none of them may be walked
GRAM_CARRY_RAGGED = [(2, 32769, 3), (29, 565, 65), (17, 241, 129)]
GRAM_SEAMS += GRAM_CARRY_RAGGED
GRAM_FORMS = (1, 2, 3)

# (nx, ny, M): small shapes and (257, 3); the large M on the smallest shapes; 7 and 20 reach the register steps 8 and 32
PROJECT_CASES = [
    (7, 9, 3), (8, 8, 12), (5, 13, 48), (130, 67, 12), (257, 3, 64), (1, 300, 7), (257, 3, 20),
    (1, 1, 65), (7, 9, 65), (8, 8, 128), (5, 13, 256),
    (7, 9, 8), (7, 9, 17), (7, 9, 33),  # a full register step, and the first M of a step, on one wave with a lane past the end
]
PROJECT_FORMS = (0, 1)


def weights(M, K, seed=0):
    return np.random.default_rng([seed, M, K]).standard_normal((M, K))
