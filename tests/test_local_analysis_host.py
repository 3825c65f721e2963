"""The local analysis on the CPU: csim_obs_local_count against brute force, and the numpy restatement of the csim.h
block (tests/local_analysis_restatement.py) against the textbook it claims to equal in exact arithmetic: per cell, mean
and variance of an eigh-based LETKF with R_loc = diag(r / rho), and of the restatement itself under permutations of
the input order.  No GPU."""
import numpy as np
import pytest

import local_analysis_restatement as ref
from __graft_entry__ import load_package

# The bar of the equivalence test.  Measured: the largest |difference| / max(|mean|, var, 1) between the restatement and
# the eigh LETKF, and between the restatement and itself under three permutations of the input order, over every cell
# of CASES below (numpy 2.x with OpenBLAS LAPACK, x86-64) is EQUIV_MEASURED; the bar is 16 times that, the margin for
# other LAPACK builds.  The reference is the eigh LETKF.  DESIGN 7s records the same figure.  Per case, against the LETKF
# and under permutations: 2.7e-15, 3.4e-15; 3.5e-14, 2.5e-15; 1.7e-14, 1.4e-15; 2.0e-14, 1.6e-15; 8.7e-15, 6.7e-15;
# 6.3e-15, 6.1e-16.
EQUIV_MEASURED = 3.524e-14
EQUIV_BAR = 16 * EQUIV_MEASURED

# M, nx, ny, loc, nobs: M of the issue's set, grids up to 24 x 20, both radii, r in [0.01, 10]
CASES = [(2, 12, 10, 2.5, 14), (5, 24, 20, 2.5, 60), (17, 24, 20, 4.0, 40), (64, 16, 12, 4.0, 30),
         (5, 9, 7, 4.0, 25), (17, 13, 20, 2.5, 50)]


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    return pkg


COUNT_CASES = [(8, 6, 1, 1), (8, 6, 2, 0), (8, 6, 0, 3), (8, 6, 30, 2), (8, 6, 3, 40), (1, 1, 0, 0), (1, 7, 5, 2),
               (37, 21, 4, 4), (16, 16, 7, 3)]


@pytest.mark.parametrize("case", COUNT_CASES, ids=[f"{c[0]}x{c[1]}_l{c[2]}_{c[3]}" for c in COUNT_CASES])
def test_local_count_is_the_rectangle_count(csim, case):
    """corners, edges, a duplicated cell, half-widths beyond the grid, against one loop per observation"""
    nx, ny, lx, ly = case
    rng = np.random.default_rng(nx * 100 + ny + lx)
    n = 40
    i, j = rng.integers(1, nx + 1, n), rng.integers(1, ny + 1, n)
    i[:6], j[:6] = [1, nx, 1, nx, 1, (nx + 1) // 2], [1, ny, ny, 1, (ny + 1) // 2, 1]
    i[6], j[6] = i[7], j[7]
    want = ref.local_count(nx, ny, i, j, lx, ly)
    count, most = csim.obs_local_count(nx, ny, i, j, lx, ly)
    assert count.dtype == np.int32 and np.array_equal(count, want) and most == want.max()
    assert most >= 2          # the duplicated cell
    if lx >= nx - 1 and ly >= ny - 1:
        assert (count == n).all()


def test_local_count_edges_and_errors(csim):
    L, C = csim.lib(), csim.C
    count, most = csim.obs_local_count(5, 4, [], [], 2, 2)
    assert most == 0 and not count.any()
    ip = lambda v: np.asarray(v, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    m = C.c_int(-1)
    assert L.csim_obs_local_count(5, 4, 1, ip([3]), ip([2]), 1, 1, None, C.byref(m)) == 0 and m.value == 1
    assert L.csim_obs_local_count(5, 4, 1, ip([3]), ip([2]), 1, 1, None, None) == 0
    for args in ((0, 4, 1, ip([3]), ip([2]), 1, 1), (5, 0, 1, ip([3]), ip([2]), 1, 1), (5, 4, -1, ip([3]), ip([2]), 1, 1),
                 (5, 4, 1, None, ip([2]), 1, 1), (5, 4, 1, ip([3]), None, 1, 1), (5, 4, 1, ip([3]), ip([2]), -1, 1),
                 (5, 4, 1, ip([3]), ip([2]), 1, -1), (5, 4, 1, ip([6]), ip([2]), 1, 1), (5, 4, 1, ip([3]), ip([0]), 1, 1)):
        assert L.csim_obs_local_count(*args, None, C.byref(m)) == 1
    assert csim.LOCAL_MAX_OBS == ref.MAX_OBS == 64 and csim.LOCAL_MAX_DOUBLES == ref.MAX_DOUBLES == 4096
    assert csim.LOCAL_MAX_PRIOR_DOUBLES == ref.MAX_PRIOR_DOUBLES == 1 << 26
    assert L.csim_abi_version() == 1


def test_the_restatement_of_one_observation_is_the_serial_filter():
    """one observation, the observed cell (rho = 1): the block and the serial filter of csim_ensemble_assimilate are the
    same operations, so their restatements give the same bits"""
    import obsop_restatement as obsop
    import screen_restatement as screen
    rng = np.random.default_rng(4)
    X = rng.standard_normal((6, 9, 11))
    rho = np.ones((1, 1))
    i, j, y, r = np.array([4]), np.array([3]), np.array([0.3]), np.array([0.7])
    for lam, t in ((1.0, None), (1.1, 2)):
        got = ref.analysis(X, rho, i, j, None, y, r, lam, t)
        want = obsop.analysis(X, rho, np.zeros(1, dtype=np.int32), i, j, screen.point_taps(1), y, r, lam, t)
        assert np.array_equal(got.view(np.int64), want.view(np.int64))


def equivalence_errors(csim, case):
    """over every cell of one case with a non-empty list: the largest |difference| / max(|mean|, var, 1) against the
    LETKF, and against the restatement under three permutations"""
    M, nx, ny, loc, nobs = case
    rng = np.random.default_rng(1000 * M + nx)
    rho = csim.ensemble_gc_table(1.0, 1.0, loc, nx, ny)
    X = rng.standard_normal((M, ny + 2, nx + 2)) + rng.standard_normal((1, ny + 2, nx + 2))
    i, j = rng.integers(1, nx + 1, nobs).astype(np.int32), rng.integers(1, ny + 1, nobs).astype(np.int32)
    i[1], j[1] = i[0], j[0]
    r = 10.0 ** rng.uniform(-2, 1, nobs)
    y = rng.standard_normal(nobs)
    H = ref.priors(X, None, i, j)
    perms = [rng.permutation(nobs) for _ in range(3)]
    e_letkf = e_perm = 0.0
    longest = 0
    for cj in range(1, ny + 1):
        for ci in range(1, nx + 1):
            obs, re = ref.local_list(ci, cj, rho, i, j, r)
            if not obs:
                continue
            longest = max(longest, len(obs))
            z = ref.cell_update(X[:, cj, ci], H[obs], y[obs], re)
            m, v = z.mean(), z.var(ddof=1)
            scale = max(abs(m), v, 1.0)
            lm, lv = ref.letkf_cell(X[:, cj, ci], H[obs], y[obs], re)
            e_letkf = max(e_letkf, abs(m - lm) / scale, abs(v - lv) / scale)
            for p in perms:
                po, pre = ref.local_list(ci, cj, rho, i[p], j[p], r[p])
                zp = ref.cell_update(X[:, cj, ci], H[p][po], y[p][po], pre)
                assert sorted(p[po]) == obs
                e_perm = max(e_perm, abs(m - zp.mean()) / scale, abs(v - zp.var(ddof=1)) / scale)
    return e_letkf, e_perm, longest


@pytest.mark.parametrize("case", CASES, ids=[f"M{c[0]}_{c[1]}x{c[2]}_loc{c[3]}" for c in CASES])
def test_restatement_is_the_letkf_and_order_independent(csim, case):
    e_letkf, e_perm, longest = equivalence_errors(csim, case)
    print(f"case {case}: lists up to {longest}; against the LETKF {e_letkf:.3e}, under permutations {e_perm:.3e}")
    assert longest >= 3
    assert e_letkf <= EQUIV_BAR and e_perm <= EQUIV_BAR
