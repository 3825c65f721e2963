"""The LETKF on the GPU (csim_ensemble_assimilate_letkf), members and the per-node record bit for bit against the numpy
restatement of the csim.h block (tests/letkf_restatement.py, which tests/test_letkf_host.py holds against a dense eigh
LETKF): lattices that fit and that end short, one node per cell and one node per axis, the register / LDS seam of the
cell pass and the three storage forms of the eigensolver, every forced form, point and linear networks, idle and
non-finite nodes, a network beyond the local analysis's limits, the record, a cycle that only enqueues, and the Kalman
check against csim_ensemble_assimilate_local.  Everything is compared through integer views; ghost rings and the truth
member are part of every comparison.  The grids are small: what is under test goes per node, per patch and per cell."""
import numpy as np
import pytest

import letkf_restatement as ref
import obsnet_restatement as obsnet
import screen_restatement as screen
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

LOC = 2.5   # half-widths (4, 4) on a unit grid
FACTOR = 8  # the project's allowance over the eigh version's own distance (tests/test_etkf_host.py)


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


@pytest.fixture(scope="module")
def eig(csim):
    return lambda C: csim.sym_eigen(C, order="round_robin")


def same_bits(got, want):
    """the same 64-bit patterns, where a NaN matches any NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.int64), want[ok].view(np.int64))


def exact_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def same_info(got, want):
    return (exact_bits(got.dfs, want.dfs) and np.array_equal(got.count, want.count)
            and np.array_equal(got.sweeps, want.sweeps) and np.array_equal(got.status, want.status))


def ensemble(csim, X, nx, ny, bcs="dddd"):
    e = csim.Ensemble(X.shape[0], nx, ny, 1.0, 1.0, csim.bc_codes(bcs), 0.5)
    e.upload_all(X)
    return e


def truth_of(where, B):
    return {None: None, "first": 0, "middle": B // 2}[where]


def cells_of(rng, nx, ny, s, nobs):
    """random cells; the first ones on a node, between nodes, in a corner (a clipped window) and two on one cell"""
    i, j = rng.integers(1, nx + 1, nobs), rng.integers(1, ny + 1, nobs)
    fixed = [(min(1 + s, nx), min(1 + s, ny)), (min(2, nx), min(3, ny)), (nx, ny), (1, ny), (min(3, nx), min(2, ny)),
             (min(3, nx), min(2, ny))]
    for o, (a, b) in enumerate(fixed[:nobs]):
        i[o], j[o] = a, b
    return i.astype(np.int32), j.astype(np.int32)


def run_case(csim, eig, nx, ny, s, M, where, lam, nobs=12, seed=0, kind="point", forms=((0, 0),)):
    """one ensemble and network, the restatement once, the analysis once per (eigen_form, letkf_form)"""
    B = M if where is None else M + 1
    t = truth_of(where, B)
    rng = np.random.default_rng(1000 * M + 10 * nx + s + seed)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    r = rng.uniform(0.05, 2.0, nobs)
    taps = None
    if kind == "bilinear":
        x, y = rng.uniform(1, nx, nobs), rng.uniform(1, ny, nobs)
        x[:3], y[:3] = [1.0, nx, 1.25], [1.0, ny, ny - 0.25]
        i, j, taps = csim.bilinear_taps(nx, ny, x, y)
        taps = tuple(taps)
    else:
        i, j = cells_of(rng, nx, ny, s, nobs)
        if kind == "box":
            i, j, taps = csim.box_taps(nx, ny, i, j, 1, 1)
            taps = tuple(taps)
    yv = rng.standard_normal(nobs)
    rho = csim.ensemble_gc_table(1.0, 1.0, LOC, nx, ny)
    want, info, _ = ref.analysis(X, rho, i, j, taps, yv, r, lam, t, s, eig)
    assert not same_bits(want, X)
    for eform, lform in forms:
        e = ensemble(csim, X, nx, ny)
        e.set_option("eigen_form", eform)
        e.set_option("letkf_form", lform)
        net = e.obs_network(i, j, r, LOC, taps=taps)
        net.set_values(yv)
        e.assimilate_letkf(net, inflation=lam, truth_member=t, spacing=s)
        A = e.download_all()
        assert same_bits(A, want), (eform, lform, np.argwhere(A != want)[:5])
        got = e.letkf_info()
        assert got.status.shape == (len(ref.axis_nodes(ny, s)), len(ref.axis_nodes(nx, s)))
        assert same_info(got, info), (eform, lform)
        assert not net.status().any()
        e.close()
    return info


# ---- 1. bits -----------------------------------------------------------------------------------------------------------

# nx, ny, s: the lattice fits exactly; a short last interval; one node per cell; patches of 3 x 3, 8 x 8 (cut by the
# grid) and one patch for the whole grid; one column
LATTICES = [(13, 9, 4), (14, 9, 4), (24, 20, 1), (24, 20, 3), (24, 20, 8), (24, 20, 100), (1, 7, 2)]


@pytest.mark.parametrize("lattice", LATTICES, ids=lambda c: f"{c[0]}x{c[1]}_s{c[2]}")
@pytest.mark.parametrize("where,lam", [(None, 1.0), ("middle", 1.1)], ids=["all_lam1", "tmiddle_lam1.1"])
def test_letkf_is_the_restatement(csim, eig, lattice, where, lam):
    nx, ny, s = lattice
    info = run_case(csim, eig, nx, ny, s, 5, where, lam, nobs=12 if nx > 1 else 4)
    assert (info.status == ref.OK).any()


# the register steps' ends, the register / LDS seam of the cell pass (64 | 65) and the solver's three forms (96 | 97,
# 128 | 129); every eigen_form that admits M forced, and every letkf_form at M = 5 and 64.  Then the cell pass's other
# register steps, each full and at its first M, with one eigen_form; both letkf_forms at M = 16 and 33
MEMBERS = [(2, "first", (1, 2, 3), (0,)), (5, None, (1, 2, 3), (0, 1)), (64, "first", (1, 2, 3), (0, 1)),
           (65, None, (1, 2, 3), (0,)), (97, None, (2, 3), (0,)), (129, "middle", (3,), (0,)),
           (8, "middle", (1,), (0,)), (9, None, (1,), (0,)), (16, "first", (1,), (0, 1)), (17, "middle", (1,), (0,)),
           (33, None, (1,), (0, 1)), (49, "first", (1,), (0,))]


@pytest.mark.parametrize("case", MEMBERS, ids=lambda c: f"M{c[0]}_t{c[1]}")
def test_member_counts_and_forced_forms(csim, eig, case):
    M, where, eforms, lforms = case
    assert all(csim.sym_eigen_device_form(M, f)[0] == f for f in eforms)
    forms = [(0, lf) for lf in lforms] + [(ef, lforms[-1]) for ef in eforms]
    run_case(csim, eig, 14, 9, 4, M, where, 1.1 if M in (5, 65) else 1.0, forms=forms)


@pytest.mark.parametrize("kind", ["bilinear", "box"])
def test_linear_networks(csim, eig, kind):
    run_case(csim, eig, 13, 9, 4, 8, "first", 1.1, kind=kind, seed=3)


# ---- 2. idle and non-finite nodes ----------------------------------------------------------------------------------------

def test_idle_nodes_beside_active_ones(csim, eig):
    """24 x 20 with s = 3: four observations in one corner region, one of them masked and one rejected by the background
    check; most nodes have no local observation.  A cell whose four nodes are idle keeps the bits it had after the
    inflation"""
    nx, ny, s, M, lam, tol = 24, 20, 3, 8, 1.1, 4.0
    rng = np.random.default_rng(71)
    X = rng.standard_normal((M, ny + 2, nx + 2))
    i = np.array([4, 5, 20, 12], dtype=np.int32)
    j = np.array([4, 6, 16, 10], dtype=np.int32)
    r = np.array([0.5, 1.0, 0.7, 0.3])
    hb, vb = obsnet.mv(X, None, i, j)
    y = hb + 0.3 * np.sqrt(vb + r)
    y[2] = hb[2] + 50.0 * np.sqrt(vb[2] + r[2])      # rejected
    mask = np.array([1, 1, 1, 0], dtype=np.uint8)    # the last one masked
    st = screen.statuses(y, hb, vb, r, tol, mask)
    assert st.tolist() == [screen.USED, screen.USED, screen.REJECTED, screen.INACTIVE]
    rho = csim.ensemble_gc_table(1.0, 1.0, LOC, nx, ny)
    want, info, Xi = ref.analysis(X, rho, i, j, None, y, r, lam, None, s, eig, st)
    e = ensemble(csim, X, nx, ny)
    net = e.obs_network(i, j, r, LOC)
    net.set_values(y)
    net.set_active(mask)
    e.assimilate_letkf(net, inflation=lam, spacing=s, screen=tol)
    A = e.download_all()
    assert same_bits(A, want) and np.array_equal(net.status(), st)
    got = e.letkf_info()
    assert same_info(got, info)
    assert (got.status == ref.IDLE).sum() > 4 and (got.status == ref.OK).sum() >= 4
    # the nodes around the rejected and the masked observation are idle; cells between four idle nodes keep their bits
    assert got.status[5, 6] == ref.IDLE and got.status[3, 4] == ref.IDLE
    kept = 0
    for cj in range(1, ny + 1):
        for ci in range(1, nx + 1):
            node, beta = ref.blend(nx, ny, s, ci, cj)
            if all(info.status.ravel()[n] == ref.IDLE for n, b in zip(node, beta) if b != 0.0):
                assert np.array_equal(A[:, cj, ci].view(np.int64), Xi[:, cj, ci].view(np.int64))
                kept += 1
    assert kept > 100
    e.close()


def test_a_nan_prior_marks_its_nodes(csim, eig):
    """a NaN cell of one member under an observation: the nodes whose list holds it are NONFINITE and letkf_info raises;
    the cells that only those nodes feed keep their bits, the others are the restatement's"""
    nx, ny, s, M = 24, 20, 3, 6
    rng = np.random.default_rng(72)
    X = rng.standard_normal((M, ny + 2, nx + 2))
    i = np.array([7, 20, 19], dtype=np.int32)
    j = np.array([7, 15, 13], dtype=np.int32)
    r = np.array([0.5, 1.0, 0.7])
    y = rng.standard_normal(3)
    X[2, 7, 7] = np.nan
    rho = csim.ensemble_gc_table(1.0, 1.0, LOC, nx, ny)
    want, info, _ = ref.analysis(X, rho, i, j, None, y, r, 1.0, None, s, eig)
    assert (info.status == ref.NONFINITE).sum() >= 4 and (info.status == ref.OK).sum() >= 4
    e = ensemble(csim, X, nx, ny)
    net = e.obs_network(i, j, r, LOC)
    net.set_values(y)
    e.assimilate_letkf(net, spacing=s)
    A = e.download_all()
    assert same_bits(A, want)
    with pytest.raises(csim.CsimError) as ei:
        e.letkf_info()
    assert ei.value.code == 4 and same_info(e.letkf_last, info)
    near = np.zeros((ny + 2, nx + 2), dtype=bool)
    near[4:11, 4:11] = True          # between the nodes at 4, 7 and 10: only non-finite nodes
    assert np.array_equal(A[:, near].view(np.int64), X[:, near].view(np.int64))
    assert not same_bits(A, X)
    e.close()


# ---- 3. beyond the local analysis's limits ---------------------------------------------------------------------------------

def test_more_windows_over_a_cell_than_the_local_analysis_takes(csim, eig):
    """100 observations on 24 x 20 with a loc whose windows cover the grid: more than 64 over one cell"""
    nx, ny, s, M, loc, nobs = 24, 20, 8, 5, 20.0, 100
    rng = np.random.default_rng(73)
    X = rng.standard_normal((M, ny + 2, nx + 2))
    i, j = cells_of(rng, nx, ny, s, nobs)
    r = rng.uniform(0.5, 2.0, nobs)
    y = rng.standard_normal(nobs)
    rho = csim.ensemble_gc_table(1.0, 1.0, loc, nx, ny)
    e = ensemble(csim, X, nx, ny)
    net = e.obs_network(i, j, r, loc)
    net.set_values(y)
    assert net.local_info() > 64
    with pytest.raises(csim.CsimError) as ei:
        e.assimilate_local(net)
    assert ei.value.code == 5
    assert exact_bits(e.download_all(), X)
    e.assimilate_letkf(net, spacing=s)
    want, info, _ = ref.analysis(X, rho, i, j, None, y, r, 1.0, None, s, eig)
    assert same_bits(e.download_all(), want) and same_info(e.letkf_info(), info)
    assert info.count.max() > 64
    e.close()


# ---- 4. the record, and a cycle that only enqueues ---------------------------------------------------------------------------

def test_recorded_analysis(csim, eig):
    nx, ny, s, B, t, nobs = 14, 9, 4, 6, 0, 10
    rng = np.random.default_rng(74)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j = cells_of(rng, nx, ny, s, nobs)
    r = rng.uniform(0.05, 2.0, nobs)
    y = rng.standard_normal(nobs)
    rho = csim.ensemble_gc_table(1.0, 1.0, LOC, nx, ny)
    e = ensemble(csim, X, nx, ny)
    net = e.obs_network(i, j, r, LOC, log_cycles=1)
    net.set_values(y)
    e.assimilate_letkf(net, inflation=1.05, truth_member=t, record=True, spacing=s)
    A = e.download_all()
    want, _, _ = ref.analysis(X, rho, i, j, None, y, r, 1.05, t, s, eig)
    assert same_bits(A, want)
    f = net.fetch()
    hb, vb = obsnet.mv(X, t, i, j)
    ha, va = obsnet.mv(A, t, i, j)
    assert same_bits(f.bg_mean, hb) and same_bits(f.bg_var, vb) and same_bits(f.post_mean, ha) and same_bits(f.post_var, va)
    log = net.log()
    rec = obsnet.cycle(y, hb, vb, ha, va, r)
    assert len(log) == 1 and all(exact_bits(log[0][k], rec[k]) for k in obsnet.FIELDS), (log[0], rec)
    with pytest.raises(csim.CsimError) as ei:     # the log is full: raised before anything is enqueued
        e.assimilate_letkf(net, truth_member=t, record=True, spacing=s)
    assert ei.value.code == 4 and exact_bits(e.download_all(), A)
    e.close()


def test_three_cycles_without_a_fetch(csim, eig):
    """run -> observe -> assimilate_letkf -> perturb, three times, nothing fetched in between; then one comparison with
    the same cycle made of host round trips and the restatement"""
    nx, ny, s, B, t, nobs, seed = 14, 9, 4, 7, 3, 8, 99
    rng = np.random.default_rng(75)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    i, j = cells_of(rng, nx, ny, s, nobs)
    r = rng.uniform(0.2, 1.0, nobs)
    rho = csim.ensemble_gc_table(1.0, 1.0, LOC, nx, ny)
    phys = ([0.05] * B, [0.1] * B, [0.3] * B, [-0.2] * B)
    e = ensemble(csim, X, nx, ny)
    e.set_physics(*phys)
    net = e.obs_network(i, j, r, LOC)
    for c in range(3):
        e.run(2)
        net.observe(t, seed, c)
        e.assimilate_letkf(net, inflation=1.05, truth_member=t, spacing=s)
        e.perturb(0.05, 1.5, seed, draw=c, centered=True, truth_member=t)
    got = e.download_all()
    e.close()
    b = ensemble(csim, X, nx, ny)
    b.set_physics(*phys)
    nb = b.obs_network(i, j, r, LOC)
    for c in range(3):
        b.run(2)
        nb.observe(t, seed, c)
        Xc = b.download_all()
        want, _, _ = ref.analysis(Xc, rho, i, j, None, nb.fetch().y, r, 1.05, t, s, eig)
        b.upload_all(want)
        b.perturb(0.05, 1.5, seed, draw=c, centered=True, truth_member=t)
    assert same_bits(got, b.download_all())
    b.close()


# ---- 5. errors -------------------------------------------------------------------------------------------------------------

def test_errors_leave_everything_as_it_was(csim):
    nx, ny, M = 14, 9, 4
    rng = np.random.default_rng(76)
    X = rng.standard_normal((M, ny + 2, nx + 2))
    e = ensemble(csim, X, nx, ny)
    with pytest.raises(csim.CsimError) as ei:
        e.letkf_info()
    assert ei.value.code == 4
    net = e.obs_network([3, 9], [3, 5], [1.0, 1.0], LOC)
    with pytest.raises(csim.CsimError) as ei:       # no values yet
        e.assimilate_letkf(net, spacing=4)
    assert ei.value.code == 4
    net.set_values([0.1, -0.2])
    for bad, code in ((0, 1), (-3, 1)):
        with pytest.raises(csim.CsimError) as ei:
            e.assimilate_letkf(net, spacing=bad)
        assert ei.value.code == code
    with pytest.raises(csim.CsimError) as ei:
        e.assimilate_letkf(net, inflation=0.5, spacing=4)
    assert ei.value.code == 1
    e.set_option("eigen_form", 1)
    assert e.get_option("letkf_form") == 0
    with pytest.raises(csim.CsimError):
        e.set_option("letkf_form", 2)
    assert exact_bits(e.download_all(), X)
    with pytest.raises(csim.CsimError) as ei:
        e.letkf_info()
    assert ei.value.code == 4
    e.close()
    # an eigen_form that does not admit M, and more nodes than the solver's batch
    big = csim.Ensemble(97, 6, 5, 1.0, 1.0, csim.bc_codes("dddd"), 0.0)
    big.set_option("eigen_form", 1)
    nb = big.obs_network([3], [3], [1.0], LOC)
    nb.set_values([0.0])
    with pytest.raises(csim.CsimError) as ei:
        big.assimilate_letkf(nb, spacing=2)
    assert ei.value.code == 5
    big.close()
    wide = csim.Ensemble(2, 300, 300, 1.0, 1.0, csim.bc_codes("dddd"), 0.0)
    nw = wide.obs_network([3], [3], [1.0], LOC)
    nw.set_values([0.0])
    assert csim.letkf_plan(2, 300, 300, 1).nodes == 90000
    with pytest.raises(csim.CsimError) as ei:
        wide.assimilate_letkf(nw, spacing=1)
    assert ei.value.code == 5
    wide.close()


# ---- 6. Kalman -------------------------------------------------------------------------------------------------------------

def test_one_node_per_cell_is_the_local_analysis(csim, eig):
    """s = 1 on 24 x 20, M = 16, 40 point observations, inside assimilate_local's limits: in exact arithmetic both are
    the LETKF's mean and variance.  The distance of this analysis from assimilate_local's, on mean and variance and
    relative to their largest magnitude, against the distance of the eigh-based numpy LETKF from it"""
    nx, ny, M, nobs = 24, 20, 16, 40
    rng = np.random.default_rng(77)
    X = rng.standard_normal((M, ny + 2, nx + 2))
    i, j = cells_of(rng, nx, ny, 1, nobs)
    r = rng.uniform(0.05, 2.0, nobs)
    y = rng.standard_normal(nobs)
    rho = csim.ensemble_gc_table(1.0, 1.0, LOC, nx, ny)
    a = ensemble(csim, X, nx, ny)
    na = a.obs_network(i, j, r, LOC)
    na.set_values(y)
    a.assimilate_local(na, inflation=1.05)
    L = a.download_all()
    a.close()
    b = ensemble(csim, X, nx, ny)
    nb = b.obs_network(i, j, r, LOC)
    nb.set_values(y)
    b.assimilate_letkf(nb, inflation=1.05, spacing=1)
    A = b.download_all()
    assert (b.letkf_info().status != ref.NOT_CONVERGED).all()
    b.close()
    E = ref.eigh_analysis(X, rho, i, j, None, y, r, 1.05, None, 1)
    ours, yard = ref.distance(A, L, None), max(ref.distance(E, L, None), M * 2.0 ** -52)
    print(f"letkf vs local: ours {ours:.3e}, eigh {yard:.3e}, allowance {FACTOR} x")
    assert ours <= FACTOR * yard
