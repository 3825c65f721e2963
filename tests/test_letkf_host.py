"""Host side of the LETKF (csim_letkf_nodes, csim_letkf_blend, csim_letkf_plan and the declarations of
csim_ensemble_assimilate_letkf and csim_ensemble_letkf_info), no GPU needed: the lattice and a cell's four nodes and
weights against the numpy restatement (tests/letkf_restatement.py) at the seams, the storage plan and the limits, every
error code, and the restatement's analysis with one node per cell against a dense numpy LETKF built on eigh.

Only the restatement's own property tests (test_restatement_*) run without the library's new symbols; the others, and
every test of tests/test_gpu_letkf.py, tests/test_gpu_letkf_cpp.py and tests/test_letkf_plan_host.py, need them."""
import numpy as np
import pytest

import letkf_restatement as ref
import local_analysis_restatement as local
from __graft_entry__ import load_package

NAMES = {"csim_ensemble_assimilate_letkf": 7, "csim_ensemble_letkf_info": 7, "csim_letkf_nodes": 7,
         "csim_letkf_blend": 7, "csim_letkf_plan": 6}
ERR_ARG, ERR_UNSUPPORTED = 1, 5
SIZES, SPACINGS = (1, 2, 5, 13, 14), (1, 2, 4, 13, 100)
FACTOR = 8  # the project's allowance over the eigh version's own distance (tests/test_etkf_host.py)
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    return pkg


def test_entry_points_are_declared_and_exported(csim):
    declared = csim.declared_symbols()
    L = csim.lib()
    for name, nargs in NAMES.items():
        assert name in declared
        assert len(getattr(L, name).argtypes) == nargs
    assert (csim.LETKF_MAX_NODES, csim.LETKF_MAX_BYTES) == (ref.MAX_NODES, ref.MAX_BYTES)
    assert (csim.LETKF_OK, csim.LETKF_IDLE, csim.LETKF_NONFINITE, csim.LETKF_NOT_CONVERGED) == (0, 1, 2, 3)


# ---- the lattice and the blend -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", SPACINGS)
@pytest.mark.parametrize("nx", SIZES)
def test_nodes_and_blend_are_the_restatement(csim, nx, s):
    for ny in SIZES:
        got = csim.letkf_nodes(nx, ny, s)
        nax, nay, xi, yj = ref.nodes(nx, ny, s)
        assert (got.nax, got.nay, got.xi.tolist(), got.yj.tolist()) == (nax, nay, xi, yj)
        assert xi[0] == 1 and xi[-1] == nx and yj[0] == 1 and yj[-1] == ny
        assert all(b - a == s for a, b in zip(xi[:-2], xi[1:-1])) and (nax < 2 or 1 <= xi[-1] - xi[-2] <= s)
        for j in range(1, ny + 1):
            for i in range(1, nx + 1):
                b = csim.letkf_blend(nx, ny, s, i, j)
                node, beta = ref.blend(nx, ny, s, i, j)
                assert b.node.tolist() == node
                assert np.array_equal(b.beta.view(np.int64), np.asarray(beta).view(np.int64))
                assert all(0 <= n < nax * nay for n in node) and (b.beta >= 0).all()
                assert abs(b.beta.sum() - 1.0) <= 2 * ULP
                if i in xi and j in yj:   # a cell on a node: that node alone, (1, 0, 0, 0) or its permutation at the last
                    assert sorted(b.beta.tolist()) == [0.0, 0.0, 0.0, 1.0]
                    assert b.node[int(np.argmax(b.beta))] == yj.index(j) * nax + xi.index(i)


@pytest.mark.parametrize("nx,ny,s", [(13, 9, 4), (14, 5, 4), (5, 14, 2), (1, 13, 4), (13, 13, 100)])
def test_a_constant_weight_field_comes_back_constant(csim, nx, ny, s):
    """the blend of a field that has the same value at every node is that value, within the rounding of the four
    products and three sums"""
    c = 0.7304
    for j in range(1, ny + 1):
        for i in range(1, nx + 1):
            b = csim.letkf_blend(nx, ny, s, i, j)
            v = 0.0
            for n in range(4):
                if b.beta[n] != 0.0:
                    v = v + b.beta[n] * c
            assert abs(v - c) <= 4 * ULP * c


# ---- the plan and the limits -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,nx,ny,s", [(2, 1, 1, 1), (5, 14, 9, 4), (64, 512, 512, 8), (96, 64, 64, 4), (97, 64, 64, 4),
                                       (256, 256, 256, 16), (64, 256, 256, 1)])
def test_plan_is_the_restatement(csim, M, nx, ny, s):
    nax, nay, _, _ = ref.nodes(nx, ny, s)
    got = csim.letkf_plan(M, nx, ny, s)
    assert got == (nax * nay, ref.plan_bytes(M, nax * nay))


def test_limits_of_the_measured_networks(csim):
    """what the limits mean for the networks of the write-up: 64 members on 512^2 fit from spacing 8, on 256^2 from
    spacing 4; 256 members on 256^2 from spacing 16; one node per cell is for small grids"""
    fits = lambda M, n, s: (csim.letkf_plan(M, n, n, s).nodes <= csim.LETKF_MAX_NODES
                            and csim.letkf_plan(M, n, n, s).bytes <= csim.LETKF_MAX_BYTES)
    assert not fits(64, 512, 4) and fits(64, 512, 8) and fits(64, 256, 4) and fits(64, 256, 8)
    assert not fits(256, 256, 8) and fits(256, 256, 16)
    assert not fits(16, 256, 1) and csim.letkf_plan(16, 256, 256, 1).nodes == 65536
    assert fits(16, 24, 1)


def test_error_codes(csim):
    L = csim.lib()
    import ctypes as C
    nodes, nbytes = C.c_long(), C.c_longlong()
    node, beta = (C.c_int * 4)(), (C.c_double * 4)()
    for args in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, -2)):
        assert L.csim_letkf_nodes(*args, None, None, None, None) == ERR_ARG
        assert L.csim_letkf_plan(4, *args, C.byref(nodes), C.byref(nbytes)) == ERR_ARG
        assert L.csim_letkf_blend(*args, 1, 1, node, beta) == ERR_ARG
    for i, j in ((0, 1), (6, 1), (1, 0), (1, 6)):
        assert L.csim_letkf_blend(5, 5, 2, i, j, node, beta) == ERR_ARG
    assert L.csim_letkf_blend(5, 5, 2, 1, 1, None, beta) == ERR_ARG and L.csim_letkf_blend(5, 5, 2, 1, 1, node, None) == ERR_ARG
    assert L.csim_letkf_plan(1, 5, 5, 2, None, None) == ERR_ARG
    assert L.csim_letkf_plan(257, 5, 5, 2, None, None) == ERR_UNSUPPORTED
    assert L.csim_letkf_plan(256, 5, 5, 2, None, None) == 0 and L.csim_letkf_nodes(5, 5, 2, None, None, None, None) == 0
    assert L.csim_ensemble_assimilate_letkf(None, None, 1.0, -1, 0, 0.0, 4) == ERR_ARG
    assert L.csim_ensemble_letkf_info(None, None, None, None, None, None, None) == ERR_ARG


# ---- the restatement's own properties ----------------------------------------------------------------------------------

def numpy_eigen(C):
    """a stand-in eigensolver with the interface of the library's, for the tests that run without it"""
    import collections
    lam, V = np.linalg.eigh(C)
    return collections.namedtuple("E", "lambda_ V sweeps")(lam[::-1].copy(), V[:, ::-1].copy(), 1)


def small_case(seed, nx=9, ny=7, M=6, nobs=8):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((M, ny + 2, nx + 2))
    i, j = rng.integers(1, nx + 1, nobs).astype(np.int32), rng.integers(1, ny + 1, nobs).astype(np.int32)
    r, y = rng.uniform(0.2, 2.0, nobs), rng.standard_normal(nobs)
    rho = np.zeros((5, 5))
    for b in range(-2, 3):
        for a in range(-2, 3):
            rho[b + 2, a + 2] = max(0.0, 1.0 - np.hypot(a, b) / 2.9)
    return X, rho, i, j, y, r


def test_restatement_without_observations_near_a_cell_keeps_its_bits():
    X, rho, i, j, y, r = small_case(1)
    i[:], j[:] = 2, 2
    A, info, Xi = ref.analysis(X, rho, i, j, None, y, r, 1.0, None, 3, numpy_eigen)
    assert (info.status == ref.IDLE).any() and (info.status == ref.OK).any()
    assert np.array_equal(A[:, 5:, 7:].view(np.int64), X[:, 5:, 7:].view(np.int64))
    assert not np.array_equal(A[:, 2, 2], X[:, 2, 2])
    assert (info.count[info.status == ref.IDLE] == 0).all() and (info.dfs[info.status == ref.IDLE] == 0).all()


def test_restatement_gram_is_symmetric_and_counts_its_list():
    X, rho, i, j, y, r = small_case(2)
    H = local.priors(X, None, i, j)
    obs, re = local.local_list(4, 4, rho, i, j, r)
    A = ref.node_gram(H, y, obs, re)
    assert np.array_equal(A, A.T) and A.shape == (7, 7) and len(obs) >= 1
    Z = np.array([np.append((H[o] - H[o].mean()), y[o] - H[o].mean()) / np.sqrt(q) for o, q in zip(obs, re)])
    assert np.allclose(A, Z.T @ Z, rtol=1e-12, atol=1e-12)


def test_restatement_a_nan_prior_marks_its_nodes_only():
    X, rho, i, j, y, r = small_case(3)
    i[0], j[0] = 2, 2
    X[1, 2, 2] = np.nan
    _, info, _ = ref.analysis(X, rho, i, j, None, y, r, 1.0, None, 2, numpy_eigen)
    bad = info.status == ref.NONFINITE
    assert bad[0, 0] and bad.sum() >= 1 and (info.status == ref.OK).any()


# ---- Kalman: one node per cell -------------------------------------------------------------------------------------------

def test_one_node_per_cell_is_the_dense_letkf(csim):
    """spacing 1, M = 16, 40 observations: the restatement on the library's round-robin eigensolver against a dense
    numpy LETKF of every cell on eigh (local_analysis_restatement.letkf_cell).  The yardstick is the distance of the
    eigh-based version of this analysis (letkf_restatement.eigh_analysis) from the same reference, floored at M 2^-52"""
    nx, ny, M, nobs = 12, 10, 16, 40
    rng = np.random.default_rng(16)
    X = rng.standard_normal((M, ny + 2, nx + 2))
    i, j = rng.integers(1, nx + 1, nobs).astype(np.int32), rng.integers(1, ny + 1, nobs).astype(np.int32)
    r, y = rng.uniform(0.05, 2.0, nobs), rng.standard_normal(nobs)
    rho = csim.ensemble_gc_table(1.0, 1.0, 2.5, nx, ny)
    eig = lambda C: csim.sym_eigen(C, order="round_robin")
    A, info, Xi = ref.analysis(X, rho, i, j, None, y, r, 1.05, None, 1, eig)
    assert (info.status != ref.NOT_CONVERGED).all() and info.status.shape == (ny, nx)
    E = ref.eigh_analysis(X, rho, i, j, None, y, r, 1.05, None, 1)
    H = local.priors(Xi, None, i, j)
    mean, var = Xi[:, 1:-1, 1:-1].mean(axis=0), Xi[:, 1:-1, 1:-1].var(axis=0, ddof=1)
    for cj in range(1, ny + 1):
        for ci in range(1, nx + 1):
            obs, re = local.local_list(ci, cj, rho, i, j, r)
            if obs:
                mean[cj - 1, ci - 1], var[cj - 1, ci - 1] = local.letkf_cell(Xi[:, cj, ci], H[obs], y[obs], re)

    def dist(Z):
        m, v = ref.mean_var(Z, None)
        return max(np.max(np.abs(m - mean)) / np.max(np.abs(mean)), np.max(np.abs(v - var)) / np.max(np.abs(var)))

    ours, yard = dist(A), max(dist(E), M * ULP)
    print(f"restatement vs dense LETKF: ours {ours:.3e}, eigh {yard:.3e}, allowance {FACTOR} x")
    assert ours <= FACTOR * yard
