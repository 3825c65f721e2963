"""The held-row kernels at their block, member and form seams (k_held_mv and k_held_transform of
csrc/ensemble_held.hip, the ROWS form of k_obsgram_partial of csrc/ensemble_obsgram.hip) against the numpy restatements
(tests/held_restatement.py, tests/etkf_restatement.py, tests/screen_restatement.py, tests/espace_restatement.py), bit
for bit.  The cases and their inputs are tests/held_seam_cases.py, which tests/test_held_seam_cases_host.py holds to what
it claims and whose reference it shows to tell five wrong kernels from the right one.
  a. the held analysis over the case table, both paths: rows, (mean, variance) before and after by input index, status
     bytes and members; full blocks, second and third blocks, tails of one row, M from 2 to 256 in every residue of 4
  b. the Gram matrix from rows at the column counts where the shared tile geometry changes, every form, against the
     restatement and not against the gathering kernel
  c. a held row that is not finite: what either path reports, that nothing is written, and whether the window is over
  d. one row; and nothing used with inflation 1 on a grid of three blocks
Every comparison goes through integer views.  Every test here needs csim_ensemble_assimilate_etkf_held."""
import numpy as np
import pytest

import espace_restatement as espace
import etkf_restatement as ref
import held_restatement as held
import held_seam_cases as hc
import screen_restatement as screen
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

ERR_STATE = 4
GRID = hc.GRID
FORMS = (1, 2, 3, 0)


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


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


def symmetric(A):
    return np.array_equal(A.view(np.int64), A.T.copy().view(np.int64))


def ensemble(csim, X):
    nx, ny, dx, dy, _ = GRID
    e = csim.Ensemble(X.shape[0], nx, ny, dx, dy, csim.bc_codes("dddd"), 0.5)
    e.upload_all(X)
    return e


def order_of(csim, net, i, j):
    info = net.info
    return ref.plan_order(csim.ensemble_assim_plan(i, j, info.lx, info.ly))


def hold_two_slots(csim, x, mask):
    """the ensemble at X1 and the network with slot 0 held from X0 and slot 1 from X1"""
    e = ensemble(csim, x.X0)
    net = e.obs_network(x.i, x.j, x.r, GRID[4], taps=x.taps, log_cycles=2)
    assert net.info.nlevels > 1 or len(x.i) == 1
    assert np.array_equal(order_of(csim, net, x.i, x.j), x.order)   # the network's plan is the one the cases used
    net.set_values(x.y)
    net.set_active(mask)
    net.set_slots(x.slot)
    net.hold(0, truth_member=x.t)
    e.upload_all(x.X1)
    net.hold(1, truth_member=x.t)
    return e, net


# ---- a. transform and mv at the seams --------------------------------------------------------------------------------

@pytest.mark.parametrize("c,device", hc.RUNS, ids=hc.RUN_IDS)
def test_held_analysis_at_the_block_and_member_seams(csim, c, device):
    x = hc.inputs(csim, c)
    e, net = hold_two_slots(csim, x, x.mask)
    assert exact_bits(net.held(), x.H)
    e.assimilate_etkf(net, inflation=hc.INFLATION, truth_member=x.t, record=True, screen=hc.TOL, held=True, device=device)
    W, wbar = hc.weights(csim, c, device)
    Ha = held.row_transform(x.H, W, wbar)
    got = net.held()
    assert exact_bits(got, Ha) and not exact_bits(got, x.H)
    ha, va = held.row_mv(Ha)
    f = net.fetch()
    assert exact_bits(f.bg_mean, x.hb) and exact_bits(f.bg_var, x.vb)
    assert exact_bits(f.post_mean, ha) and exact_bits(f.post_var, va)
    assert np.array_equal(net.status(), x.status)
    assert e.etkf_info().n_used == np.count_nonzero(x.status == screen.USED)
    assert exact_bits(e.download_all(), espace.transform(x.X1, W, wbar, x.t, True))
    e.close()


# ---- b. the Gram matrix from rows where the shared tile geometry changes ---------------------------------------------

@pytest.mark.parametrize("nobs", hc.GRAM_NOBS)
@pytest.mark.parametrize("cols", hc.GRAM_COLS)
def test_held_gram_at_the_geometry_seams(csim, cols, nobs):
    g = hc.gram_inputs(csim, cols, nobs)
    M = g.M
    assert hc.gram_blocks(cols) == hc.GRAM_BLOCKS[cols]
    assert csim.obs_gram_plan(M, nobs) == ref.gram_plan(M, nobs) == (-(-nobs // 64),) * 2
    e = ensemble(csim, g.X0)
    net = e.obs_network(g.i, g.j, g.r, GRID[4])
    assert net.info.nlevels > 1 and np.array_equal(order_of(csim, net, g.i, g.j), g.order)
    net.set_values(g.y)
    net.set_active(g.mask)
    net.set_slots(g.slot)
    net.hold(0)
    e.upload_all(g.X1)
    net.hold(1)
    e.upload_all(g.X2)            # nothing of the current state can stand in for the rows
    H = net.held()
    assert exact_bits(H, g.H)
    A, ll, n = ref.obs_gram(H.T, g.y, g.r, g.mask == 1, g.order, loglik=True)
    assert n == int(g.mask.sum()) < nobs
    for form in FORMS:
        e.set_option("obs_gram_form", form)
        got = e.obs_gram(net, loglik=True, held=True)
        assert exact_bits(got.A, A) and exact_bits(got.loglik, ll) and got.n_used == n, form
        assert symmetric(got.A), form
    e.set_option("obs_gram_form", 0)
    bare = e.obs_gram(net, held=True)
    assert bare.loglik is None and exact_bits(bare.A, A) and bare.n_used == n
    assert exact_bits(net.held(), g.H)   # writes nothing of the network
    e.close()


# ---- c. a row that is not finite ---------------------------------------------------------------------------------------

def nan_case(csim):
    """the (65, 129) case with a NaN in one forecast member at the cell of the observation at the last plan position,
    which is the tail block's only row and is active; in the state that its slot is held from"""
    c = hc.case_of(65, 129)
    x = hc.inputs(csim, c)
    o = int(x.order[-1])
    assert c.blocks == 3 and c.last_rows == 1 and x.mask[o] == 1 and x.taps is None
    k = [m for m in range(x.B) if m != x.t][17]
    states = [x.X0.copy(), x.X1.copy()]
    states[x.slot[o]][k, x.j[o], x.i[o]] = np.nan
    H = held.assemble({0: states[0], 1: states[1]}, x.slot, lambda S: hc.operator(S, x.t, x.i, x.j, x.taps))
    bad = np.isnan(H).any(axis=1)
    assert np.array_equal(np.flatnonzero(bad), [o])   # distinct cells: one row
    clean = hc.members(x.B, GRID, 45)
    return c, x, o, states, H, clean


def hold_nan(csim, x, states, clean):
    e = ensemble(csim, states[0])
    net = e.obs_network(x.i, x.j, x.r, GRID[4])
    net.set_values(x.y)
    net.set_active(x.mask)
    net.set_slots(x.slot)
    net.hold(0, truth_member=x.t)
    e.upload_all(states[1])
    net.hold(1, truth_member=x.t)
    e.upload_all(clean)             # the state is clean, only the row is not
    return e, net


def held_call(e, net, x, device):
    return e.assimilate_etkf(net, inflation=hc.INFLATION, truth_member=x.t, held=True, device=device)


def test_a_non_finite_row_fails_the_host_analysis_and_leaves_the_window_open(csim):
    c, x, o, states, H, clean = nan_case(csim)
    e, net = hold_nan(csim, x, states, clean)
    assert same_bits(net.held(), H) and np.isnan(net.held()[o]).sum() == 1
    with pytest.raises(csim.CsimError) as ei:
        held_call(e, net, x, False)
    assert ei.value.code == ERR_STATE and "non-finite" in str(ei.value)
    assert exact_bits(e.download_all(), clean) and same_bits(net.held(), H)
    # the failed analysis has not ended the window: without its bad row, and without a new hold, the analysis is the
    # reference's over the other rows
    mask = x.mask.copy()
    mask[o] = 0
    net.set_active(mask)
    res = held_call(e, net, x, False)
    assert res.n_used == int(mask.sum())
    A = ref.obs_gram(np.where(np.isnan(H), 0.0, H).T, x.y, x.r, mask == 1, x.order)[0]   # a row not used is not read
    assert np.isfinite(A).all()
    w = csim.etkf_weights(A, hc.INFLATION)
    assert exact_bits(e.download_all(), espace.transform(clean, w.W, w.wbar, x.t, True))
    Ha = held.row_transform(H, w.W, w.wbar)
    assert np.isnan(Ha[o]).all() and np.isfinite(np.delete(Ha, o, axis=0)).all()
    assert same_bits(net.held(), Ha)
    # now the window is over
    with pytest.raises(csim.CsimError) as ei:
        held_call(e, net, x, False)
    assert ei.value.code == ERR_STATE and "held" in str(ei.value)
    e.close()


def test_a_non_finite_row_on_the_device_path_is_reported_and_ends_the_window(csim):
    c, x, o, states, H, clean = nan_case(csim)
    e, net = hold_nan(csim, x, states, clean)
    assert held_call(e, net, x, True) is None          # the call returns
    for text in ("non-finite", "did not complete"):    # the record is fetched once; afterwards there is no valid info
        with pytest.raises(csim.CsimError) as ei:
            e.etkf_info()
        assert ei.value.code == ERR_STATE and text in str(ei.value)
    # k_held_transform returned early in all three blocks, the members' transform too
    assert exact_bits(e.download_all(), clean) and same_bits(net.held(), H)
    # held_done is unconditional there: the window is over, with or without the bad row
    mask = x.mask.copy()
    mask[o] = 0
    net.set_active(mask)
    for device in (True, False):
        with pytest.raises(csim.CsimError) as ei:
            held_call(e, net, x, device)
        assert ei.value.code == ERR_STATE and "held" in str(ei.value)
    assert exact_bits(e.download_all(), clean) and same_bits(net.held(), H)
    # new holds from the clean state open the next one
    net.hold(0, truth_member=x.t), net.hold(1, truth_member=x.t)
    held_call(e, net, x, True)
    assert e.etkf_info().n_used == int(mask.sum())
    assert not exact_bits(e.download_all(), clean)
    e.close()


# ---- d. rows that do not change ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_nothing_used_and_no_inflation_keeps_every_bit_of_three_blocks(csim, device):
    c = hc.case_of(65, 129)
    x = hc.inputs(csim, c)
    e, net = hold_two_slots(csim, x, np.zeros(c.nobs, dtype=np.uint8))
    e.assimilate_etkf(net, truth_member=x.t, held=True, device=device)
    info = e.etkf_info()
    assert info.n_used == 0 and info.chi2 == 0.0
    assert exact_bits(e.download_all(), x.X1) and exact_bits(net.held(), x.H)
    assert (net.status() == screen.INACTIVE).all()
    e.close()
