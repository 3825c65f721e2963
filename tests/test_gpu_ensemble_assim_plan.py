"""The two ways into the ensemble analysis, csim_ensemble_assimilate and the observation networks, on one plan
(csrc/assim_plan.cpp): with two bad arguments in one call the check that comes first in each entry point's own order
fires, with its code and text, and nothing is enqueued; and both ways give the same levels, members and diagnostics on
a plan with a shared cell, a pair of observations exactly 2 lx apart and a pair 2 lx + 1 apart."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 4  # CSIM_ERR_ARG, CSIM_ERR_STATE
NX, NY = 8, 6
NAN = float("nan")

LOC = "loc must be finite and > 0"
INFLATION = "inflation must be finite and >= 1"
TRUTH = "truth_member out of range"
ORDERED = "ordered must be 0 or 1"
TWO = "the analysis needs at least two forecast members"
OUTSIDE = "observation outside the interior"
VALUE = "observation value must be finite"
VARIANCE = "observation error variance must be finite and > 0"
NOBS0 = "nobs must be >= 0"
NOBS1 = "nobs must be >= 1"
NULL_OBS = "null observation array"
NULL_TAPS = "null tap array"
LOG = "log_cycles must be in 0 .. 65536"
START0 = "start[0] must be 0"
BEYOND = "tap beyond the localisation half-width of its anchor"
OTHER = "the network belongs to another ensemble"
RECORD = "record must be 0 or 1"
TOL = "tol must be finite and >= 0"
NO_VALUES = ("csim_ensemble_assimilate_network: the network has no values yet "
             "(csim_obs_network_set_values or csim_obs_network_observe)")
NO_LOG = "csim_ensemble_assimilate_network: the network has no log"


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    return pkg


@pytest.fixture(scope="module")
def ens(csim):
    """three members of 8 x 6 (member 1 serves as the truth), two members for the calls that need M < 2, and a
    network of each; all closed at the end"""
    rng = np.random.default_rng(5)
    three = csim.Ensemble(3, NX, NY, 1.0, 1.0, (0, 0, 0, 0))
    three.upload_all(rng.standard_normal((3, NY + 2, NX + 2)))
    two = csim.Ensemble(2, NX, NY, 1.0, 1.0, (0, 0, 0, 0))
    two.upload_all(rng.standard_normal((2, NY + 2, NX + 2)))
    nets = [e.obs_network([2, 6], [3, 4], 0.5, 1.2) for e in (three, two)]
    yield three, two, nets[0], nets[1]
    three.close(), two.close()


def ints(v):
    return (C.c_int * len(v))(*v)


def dbls(v):
    return (C.c_double * len(v))(*v)


I2, J2, Y2, R2 = [2, 6], [3, 4], [0.5, -0.5], [0.5, 1.0]

# csim_ensemble_assimilate(e, nobs, i, j, y, r, loc, inflation, truth_member, ordered): two bad arguments each, and
# the text of the one whose check comes first
ONE_SHOT = [
    ("nobs_before_loc", 3, (-1, I2, J2, Y2, R2, 0.0, 1.0, 1, 0), NOBS0),
    ("null_before_loc", 3, (2, None, J2, Y2, R2, 0.0, 1.0, 1, 0), NULL_OBS),
    ("loc_before_outside", 3, (2, [0, 6], J2, Y2, R2, 0.0, 1.0, 1, 0), LOC),
    ("loc_before_inflation", 3, (2, I2, J2, Y2, R2, NAN, 0.5, 1, 0), LOC),
    ("inflation_before_truth", 3, (2, I2, J2, Y2, R2, 1.2, 0.5, 3, 0), INFLATION),
    ("truth_before_ordered", 3, (2, I2, J2, Y2, R2, 1.2, 1.0, -2, 2), TRUTH),
    ("ordered_before_members", 2, (2, I2, J2, Y2, R2, 1.2, 1.0, 0, 2), ORDERED),
    ("members_before_outside", 2, (2, [2, 9], J2, Y2, R2, 1.2, 1.0, 0, 0), TWO),
    ("earlier_r_before_later_cell", 3, (2, [2, 9], J2, Y2, [0.0, 1.0], 1.2, 1.0, 1, 0), VARIANCE),
    ("earlier_r_before_later_y", 3, (2, I2, J2, [0.5, NAN], [-1.0, 1.0], 1.2, 1.0, 1, 0), VARIANCE),
    ("earlier_y_before_later_cell", 3, (2, [2, 6], [3, 7], [NAN, 0.5], R2, 1.2, 1.0, 1, 0), VALUE),
    ("cell_before_y_and_r", 3, (2, [2, 6], [3, 0], [0.5, NAN], [0.5, NAN], 1.2, 1.0, 1, 0), OUTSIDE),
    ("y_before_r", 3, (2, I2, J2, [0.5, NAN], [0.5, 0.0], 1.2, 1.0, 1, 0), VALUE),
]


@pytest.mark.parametrize("case", ONE_SHOT, ids=[c[0] for c in ONE_SHOT])
def test_assimilate_first_error_wins(csim, ens, case):
    _, members, (nobs, i, j, y, r, loc, lam, t, ordered), text = case
    e = ens[0] if members == 3 else ens[1]
    before = e.checksums()
    nl = C.c_int(-7)
    out = [dbls([0.0, 0.0]) for _ in range(4)]
    rc = csim.lib().csim_ensemble_assimilate(e._h, nobs, i and ints(i), ints(j), dbls(y), dbls(r), loc, lam, t, ordered,
                                             *out, C.byref(nl))
    assert (rc, csim.lib().csim_last_error().decode()) == (ARG, text)
    assert nl.value == -7 and e.checksums() == before


# one tap per observation, the cell itself: start, di, dj, w
TAPS = ([0, 1, 2], [0, 0], [0, 0], [1.0, 1.0])

# csim_obs_network_create[_linear](e, nobs, i, j, [taps,] r, loc, ordered, log_cycles)
CREATE = [
    ("nobs_before_loc", (0, I2, J2, TAPS, R2, 0.0, 0, 0), NOBS1),
    ("null_before_loc", (2, I2, None, TAPS, R2, 0.0, 0, 0), NULL_OBS),
    ("loc_before_ordered", (2, I2, J2, TAPS, R2, -1.0, 2, 0), LOC),
    ("ordered_before_log", (2, I2, J2, TAPS, R2, 1.2, 2, -1), ORDERED),
    ("log_before_r", (2, I2, J2, TAPS, [0.5, NAN], 1.2, 0, -1), LOG),
    ("log_before_outside", (2, [2, 9], J2, TAPS, R2, 1.2, 0, 65537), LOG),
    ("earlier_r_before_later_cell", (2, [2, 9], J2, TAPS, [float("inf"), 1.0], 1.2, 0, 0), VARIANCE),
    ("earlier_cell_before_later_r", (2, [0, 6], J2, TAPS, [0.5, 0.0], 1.2, 0, 0), OUTSIDE),
    ("cell_before_r", (2, I2, [3, 7], TAPS, [0.5, -1.0], 1.2, 0, 0), OUTSIDE),
]
# with taps only: the observations' own checks come before those of the taps, and among the taps' checks start first
CREATE_LINEAR = [
    ("null_taps_before_loc", (2, I2, J2, (None, [0, 0], [0, 0], [1.0, 1.0]), R2, 0.0, 0, 0), NULL_TAPS),
    ("log_before_start", (2, I2, J2, ([1, 1, 2],) + TAPS[1:], R2, 1.2, 0, -1), LOG),
    ("r_before_start", (2, I2, J2, ([1, 1, 2],) + TAPS[1:], [0.5, 0.0], 1.2, 0, 0), VARIANCE),
    ("r_before_tap", (2, I2, J2, (TAPS[0], [3, 0], [0, 0], TAPS[3]), [0.5, 0.0], 1.2, 0, 0), VARIANCE),
    ("cell_before_start", (2, [2, 9], J2, ([1, 1, 2],) + TAPS[1:], R2, 1.2, 0, 0), OUTSIDE),
    ("start_before_tap", (2, I2, J2, ([1, 1, 2], [3, 0], [0, 0], [1.0, NAN]), R2, 1.2, 0, 0), START0),
    ("tap_alone", (2, I2, J2, (TAPS[0], [3, 0], [0, 0], TAPS[3]), R2, 1.2, 0, 0), BEYOND),
]


def create(csim, e, args, linear):
    nobs, i, j, (start, di, dj, w), r, loc, ordered, log_cycles = args
    h = C.c_void_p(1)
    head = (e._h, nobs, ints(i), j and ints(j))
    tail = (dbls(r), loc, ordered, log_cycles, C.byref(h))
    if linear:
        rc = csim.lib().csim_obs_network_create_linear(*head, start and ints(start), ints(di), ints(dj), dbls(w), *tail)
    else:
        rc = csim.lib().csim_obs_network_create(*head, *tail)
    return rc, csim.lib().csim_last_error().decode(), h.value


@pytest.mark.parametrize("linear", [False, True], ids=["point", "linear"])
@pytest.mark.parametrize("case", CREATE, ids=[c[0] for c in CREATE])
def test_network_create_first_error_wins(csim, ens, case, linear):
    e = ens[0]
    before = e.checksums()
    assert create(csim, e, case[1], linear) == (ARG, case[2], None)
    assert e.checksums() == before


@pytest.mark.parametrize("case", CREATE_LINEAR, ids=[c[0] for c in CREATE_LINEAR])
def test_linear_network_create_first_error_wins(csim, ens, case):
    e = ens[0]
    before = e.checksums()
    assert create(csim, e, case[1], True) == (ARG, case[2], None)
    assert e.checksums() == before


# csim_ensemble_assimilate_screened(e, n, inflation, truth_member, record, tol) on a network without values and without
# a log; `which`: the ensemble and the network
SCREENED = [
    ("other_before_inflation", (0, 3), (0.5, 1, 0, 0.0), ARG, OTHER),
    ("inflation_before_truth", (0, 2), (NAN, 3, 0, 0.0), ARG, INFLATION),
    ("truth_before_record", (0, 2), (1.0, -2, 2, 0.0), ARG, TRUTH),
    ("members_before_record", (1, 3), (1.0, 0, 2, 0.0), ARG, TWO),
    ("record_before_tol", (0, 2), (1.0, 1, 2, -1.0), ARG, RECORD),
    ("tol_before_values", (0, 2), (1.0, 1, 0, NAN), ARG, TOL),
    ("values_before_log", (0, 2), (1.0, 1, 1, 2.0), STATE, NO_VALUES),
]


@pytest.mark.parametrize("case", SCREENED, ids=[c[0] for c in SCREENED])
def test_assimilate_network_first_error_wins(csim, ens, case):
    _, (ke, kn), (lam, t, record, tol), code, text = case
    e, n = ens[ke], ens[kn]
    before = e.checksums()
    rc = csim.lib().csim_ensemble_assimilate_screened(e._h, n._h, lam, t, record, tol)
    assert (rc, csim.lib().csim_last_error().decode()) == (code, text)
    if tol == 0.0:  # the unscreened entry point is the same call
        rc = csim.lib().csim_ensemble_assimilate_network(e._h, n._h, lam, t, record)
        assert (rc, csim.lib().csim_last_error().decode()) == (code, text)
    assert e.checksums() == before


def test_network_without_a_log_after_values(csim, ens):
    """with values, the next check in line is the log's"""
    e = ens[0]
    n = e.obs_network(I2, J2, R2, 1.2)
    n.set_values(Y2)
    before = e.checksums()
    rc = csim.lib().csim_ensemble_assimilate_screened(e._h, n._h, 1.0, 1, 1, 2.0)
    assert (rc, csim.lib().csim_last_error().decode()) == (STATE, NO_LOG)
    assert e.checksums() == before


# ---- both paths, one plan -------------------------------------------------------------------------------------------

def exact_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("ordered", [False, True], ids=["first_fit", "ordered"])
def test_both_paths_one_plan(csim, ordered):
    """A 12 x 10 grid, six members with member 2 the truth, seven point observations under lx = ly = 2: 0 and 1 share a
    cell, 0 and 2 are exactly 2 lx apart (they conflict), 4 and 5 are 2 lx + 1 apart (they do not).  assimilate() and a
    network of the same arrays: the same level count, every member bit-identical, the same posterior diagnostics.  The
    network's background (hb, vb) is taken before the analysis and assimilate()'s prior when an observation's turn
    comes (csim.h), so the two are the same numbers for the observations of level 0, and are compared there."""
    nx, ny, B, t, loc = 12, 10, 6, 2, 1.2
    i = np.array([3, 3, 7, 12, 3, 8, 6], dtype=np.int32)
    j = np.array([3, 3, 3, 3, 8, 9, 7], dtype=np.int32)
    tab = csim.ensemble_gc_table(1.0, 1.0, loc, nx, ny)
    assert tab.shape == (5, 5)
    lev = csim.ensemble_assim_plan(i, j, 2, 2, ordered)
    assert lev[0] == 0 and lev[1] == 1 and lev[2] == 2 and lev[4] == lev[5] == 0 and lev.max() >= 2
    rng = np.random.default_rng(12)
    X = rng.standard_normal((B, ny + 2, nx + 2))
    y, r = rng.standard_normal(7), rng.uniform(0.1, 1.5, 7)
    a, b = (csim.Ensemble(B, nx, ny, 1.0, 1.0, (0, 0, 0, 0)) for _ in range(2))
    a.upload_all(X), b.upload_all(X)
    an = a.assimilate(i, j, y, r, loc, truth_member=t, ordered=ordered)
    net = b.obs_network(i, j, r, loc, ordered=ordered, log_cycles=1)
    net.set_values(y)
    b.assimilate_network(net, truth_member=t, record=True)
    got = net.fetch()
    A, W = a.download_all(), b.download_all()
    assert an.nlevels == net.info.nlevels == lev.max() + 1
    assert exact_bits(A, W) and exact_bits(A[t], X[t]) and not exact_bits(A, X)
    assert exact_bits(got.post_mean, an.post_mean) and exact_bits(got.post_var, an.post_var)
    first = lev == 0
    assert first.sum() >= 2
    assert exact_bits(got.bg_mean[first], an.prior_mean[first]) and exact_bits(got.bg_var[first], an.prior_var[first])
    a.close(), b.close()
