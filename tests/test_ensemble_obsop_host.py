"""Host side of the linear observations (csim_obs_network_create_linear block of include/csim.h), no GPU needed: the
two tap builders against the numpy restatement (tests/obsop_restatement.py) bit for bit, csim_obs_linear_check on a
valid set and on each violation alone, the entry points declared and exported, and nothing made without a device."""
import numpy as np
import pytest

import obsop_restatement as ref
from __graft_entry__ import load_package

NAMES = {"csim_obs_network_create_linear": 13, "csim_obs_network_taps": 2, "csim_obs_linear_check": 11,
         "csim_obs_taps_bilinear": 9, "csim_obs_taps_box": 10}


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    return pkg


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def code_of(csim, call):
    with pytest.raises(csim.CsimError) as ei:
        call()
    return ei.value.code


def test_entry_points_are_declared_and_exported(csim):
    declared = csim.declared_symbols()
    L = csim.lib()
    for name, nargs in NAMES.items():
        assert name in declared
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    assert csim.OBS_MAX_TAPS == ref.MAX_TAPS == 64
    for name in ("bilinear_taps", "box_taps", "obs_linear_check"):
        assert callable(getattr(csim, name))
    assert hasattr(csim.ObsNetwork, "ntaps")
    assert L.csim_abi_version() == 1


# ---- csim_obs_taps_bilinear ---------------------------------------------------------------------------------------

BILINEAR = [(40, 28, 1.0, 1.0), (40, 28, 40.0, 28.0), (40, 28, 40.0, 3.25), (40, 28, 7.0, 9.0), (40, 28, 39.0, 27.0),
            (40, 28, 12.3, 27.999999), (40, 28, 1.0 + 2.0 ** -52, 5.1), (40, 28, 39.99999999, 1.7), (1, 28, 1.0, 4.6),
            (40, 1, 17.4, 1.0), (1, 1, 1.0, 1.0), (2, 2, 1.5, 2.0), (3, 5, 0.1 + 0.2 + 1.0, 3.3)]


@pytest.mark.parametrize("nx,ny,x,y", BILINEAR)
def test_bilinear_against_the_restatement(csim, nx, ny, x, y):
    i, j, t = csim.bilinear_taps(nx, ny, [x], [y])
    wi, wj, wdi, wdj, ww = ref.bilinear(nx, ny, x, y)
    assert (i[0], j[0]) == (wi, wj) and list(t.start) == [0, 4]
    assert list(t.di) == wdi and list(t.dj) == wdj and same_bits(t.w, ww)
    # what the definition is for: the taps are interior, and the weights interpolate a plane exactly enough
    assert all(1 <= wi + a <= nx and 1 <= wj + b <= ny for a, b in zip(wdi, wdj))
    assert abs(sum(ww) - 1.0) <= 4 * 2.0 ** -52 and min(ww) >= 0.0
    if x == nx and nx > 1:
        assert wi == nx - 1 and ww[0] == 0.0 and ww[2] == 0.0    # fx == 1: all weight on the column nx
    if nx == 1:
        assert wdi == [0, 0, 0, 0] and ww[1] == 0.0 and ww[3] == 0.0
    if x == int(x) and y == int(y) and x < nx and y < ny:
        assert ww == [1.0, 0.0, 0.0, 0.0]


def test_bilinear_many_and_errors(csim):
    rng = np.random.default_rng(5)
    x, y = rng.uniform(1, 40, 300), rng.uniform(1, 28, 300)
    i, j, t = csim.bilinear_taps(40, 28, x, y)
    want = [ref.bilinear(40, 28, a, b) for a, b in zip(x, y)]
    assert list(i) == [v[0] for v in want] and list(j) == [v[1] for v in want]
    assert same_bits(t.w, np.concatenate([v[4] for v in want])) and list(t.start) == list(range(0, 1201, 4))
    ref_taps = ref.concat([v[2:] for v in want])
    assert np.array_equal(t.di, ref_taps[1]) and np.array_equal(t.dj, ref_taps[2])
    for bx, by in ((0.999, 5.0), (40.001, 5.0), (5.0, 0.5), (5.0, 28.5), (np.nan, 5.0), (5.0, np.inf)):
        assert code_of(csim, lambda: csim.bilinear_taps(40, 28, [bx], [by])) == 1
    L, C = csim.lib(), csim.C
    ci, a4, w4 = C.c_int(), (C.c_int * 4)(), (C.c_double * 4)()
    assert L.csim_obs_taps_bilinear(40, 28, 2.0, 2.0, None, C.byref(ci), a4, a4, w4) == 1
    assert L.csim_obs_taps_bilinear(40, 28, 2.0, 2.0, C.byref(ci), C.byref(ci), a4, a4, None) == 1
    assert L.csim_obs_taps_bilinear(0, 28, 1.0, 2.0, C.byref(ci), C.byref(ci), a4, a4, w4) == 1


# ---- csim_obs_taps_box ----------------------------------------------------------------------------------------------

BOXES = [(20, 14, 2, 2, 25), (1, 14, 2, 2, 15), (40, 14, 2, 2, 15), (20, 1, 2, 2, 15), (20, 28, 2, 2, 15),   # the sides
         (1, 1, 2, 2, 9), (40, 1, 2, 2, 9), (1, 28, 2, 2, 9), (40, 28, 2, 2, 9),                               # corners
         (2, 27, 2, 2, 16), (20, 14, 0, 0, 1), (20, 14, 3, 0, 7), (20, 14, 0, 4, 9), (20, 14, 1, 1, 9),
         (20, 14, 3, 4, 63), (20, 14, 31, 0, 40), (1, 1, 7, 7, 64)]


@pytest.mark.parametrize("i,j,a,b,count", BOXES)
def test_box_against_the_restatement(csim, i, j, a, b, count):
    gi, gj, t = csim.box_taps(40, 28, [i], [j], a, b)
    di, dj, w = ref.box(40, 28, i, j, a, b)
    assert len(w) == count and list(t.start) == [0, count] and (gi[0], gj[0]) == (i, j)
    assert list(t.di) == di and list(t.dj) == dj and same_bits(t.w, w)
    assert same_bits(t.w, np.full(count, 1.0 / count))
    cells = list(zip(dj, di))
    assert cells == sorted(cells) and len(set(cells)) == count     # rows in increasing dj, then increasing di


def test_box_refusals(csim):
    assert ref.box(40, 28, 20, 14, 4, 3) is not None                # 9 x 7 = 63 fits, 13 x 5 = 65 and 9 x 9 = 81 do not
    assert ref.box(40, 28, 20, 14, 6, 2) is None and ref.box(40, 28, 20, 14, 4, 4) is None
    assert code_of(csim, lambda: csim.box_taps(40, 28, [20], [14], 6, 2)) == 5          # 65 taps
    assert code_of(csim, lambda: csim.box_taps(40, 28, [20], [14], 4, 4)) == 5
    assert code_of(csim, lambda: csim.box_taps(200, 28, [100], [14], 32, 0)) == 5       # 65 in a row
    assert code_of(csim, lambda: csim.box_taps(40, 28, [20], [14], 2 ** 30, 2 ** 30)) == 5
    _, _, t = csim.box_taps(40, 28, [1], [1], 2 ** 30, 0)                               # clipped to the row: 40 taps
    assert list(t.start) == [0, 40]
    for bad in ((0, 14, 1, 1), (41, 14, 1, 1), (20, 0, 1, 1), (20, 29, 1, 1), (20, 14, -1, 1), (20, 14, 1, -1)):
        assert code_of(csim, lambda: csim.box_taps(40, 28, [bad[0]], [bad[1]], bad[2], bad[3])) == 1, bad
    L, C = csim.lib(), csim.C
    n, a64, w64 = C.c_int(), (C.c_int * 64)(), (C.c_double * 64)()
    assert L.csim_obs_taps_box(40, 28, 20, 14, 1, 1, None, a64, a64, w64) == 1
    assert L.csim_obs_taps_box(40, 28, 20, 14, 1, 1, C.byref(n), a64, a64, None) == 1


# ---- csim_obs_linear_check ------------------------------------------------------------------------------------------

NX, NY, LX, LY = 40, 28, 5, 3


def valid_set():
    """four observations: one tap, bilinear, a clipped box, and 64 taps with a repeated cell, a negative weight and
    taps at |di| = lx and |dj| = ly"""
    per = [([0], [0], [1.0]), tuple(ref.bilinear(NX, NY, 7.25, 9.5)[2:]), ref.box(NX, NY, 1, 1, 2, 2)]
    di = [LX, -LX, 0, 0] + [k % 7 - 3 for k in range(60)]
    dj = [0, 0, LY, -LY] + [k % 5 - 2 for k in range(60)]
    w = [0.5, -0.25, 2.0, 1e-3] + [(-1.0) ** k / 64.0 for k in range(60)]
    per.append((di, dj, w))
    i = np.array([12, 7, 1, 20], dtype=np.int32)
    j = np.array([5, 9, 1, 14], dtype=np.int32)
    return i, j, ref.concat(per)


def test_linear_check_accepts_a_valid_set(csim):
    i, j, taps = valid_set()
    assert ref.check(NX, NY, LX, LY, i, j, taps)
    csim.obs_linear_check(NX, NY, LX, LY, i, j, taps)
    assert taps[0][-1] == 1 + 4 + 9 + 64


def mutated(what):
    i, j, (start, di, dj, w) = valid_set()
    start, di, dj, w = start.copy(), di.copy(), dj.copy(), w.copy()
    if what == "tap outside the interior":       # observation 2 at (1, 1): a tap within lx of it, but in the ghost ring
        di[5] = -1
    elif what == "di = lx + 1":
        di[0], i[0] = LX + 1, 12                 # (18, 5): interior
    elif what == "dj = -(ly + 1)":
        j[0], dj[0] = 10, -(LY + 1)
    elif what == "zero taps":
        start = np.array([0, 0, 4, 13, 77], dtype=np.int32)
        di, dj, w = di[1:], dj[1:], w[1:]
    elif what == "65 taps":
        start = np.array([0, 1, 5, 14, 79], dtype=np.int32)
        di, dj, w = np.append(di, 0).astype(np.int32), np.append(dj, 0).astype(np.int32), np.append(w, 1.0)
    elif what == "nan weight":
        w[3] = np.nan
    elif what == "inf weight":
        w[77] = -np.inf
    elif what == "start[0] != 0":                # every observation keeps its number of taps
        start = start + 1
        di, dj, w = np.append(di, 0).astype(np.int32), np.append(dj, 0).astype(np.int32), np.append(w, 1.0)
    elif what == "decreasing start":
        start = np.array([0, 5, 1, 14, 78], dtype=np.int32)
    elif what == "anchor outside":
        i[3] = NX + 1
    return i, j, (start, di, dj, w)


VIOLATIONS = ["tap outside the interior", "di = lx + 1", "dj = -(ly + 1)", "zero taps", "65 taps", "nan weight",
              "inf weight", "start[0] != 0", "decreasing start", "anchor outside"]


@pytest.mark.parametrize("what", VIOLATIONS)
def test_linear_check_rejects_each_violation_alone(csim, what):
    i, j, taps = mutated(what)
    assert not ref.check(NX, NY, LX, LY, i, j, taps)
    assert code_of(csim, lambda: csim.obs_linear_check(NX, NY, LX, LY, i, j, taps)) == 1
    if what == "di = lx + 1":                   # the same set passes with a wider window: only that constraint failed
        csim.obs_linear_check(NX, NY, LX + 1, LY, i, j, taps)
    if what == "dj = -(ly + 1)":
        csim.obs_linear_check(NX, NY, LX, LY + 1, i, j, taps)


def test_linear_check_arguments(csim):
    i, j, (start, di, dj, w) = valid_set()
    L = csim.lib()
    p = [csim._ip(i), csim._ip(j), csim._ip(start), csim._ip(di), csim._ip(dj), csim._dp(w)]
    assert L.csim_obs_linear_check(NX, NY, LX, LY, 4, *p) == 0
    for k in range(6):
        q = list(p)
        q[k] = None
        assert L.csim_obs_linear_check(NX, NY, LX, LY, 4, *q) == 1
    for args in ((0, NY, LX, LY, 4), (NX, 0, LX, LY, 4), (NX, NY, -1, LY, 4), (NX, NY, LX, -1, 4), (NX, NY, LX, LY, 0),
                 (NX, NY, LX, LY, -1)):
        assert L.csim_obs_linear_check(*args, *p) == 1
    with pytest.raises(ValueError):
        csim.obs_linear_check(NX, NY, LX, LY, i, j, (start, di[:-1], dj, w))
    with pytest.raises(ValueError):
        csim.obs_linear_check(NX, NY, LX, LY, i, j, (start[:-1], di, dj, w))


def test_null_handles_are_refused_before_the_device(csim):
    L, C = csim.lib(), csim.C
    out = C.c_void_p()
    i, j, (start, di, dj, w) = valid_set()
    r = np.ones(4)
    args = [4, csim._ip(i), csim._ip(j), csim._ip(start), csim._ip(di), csim._ip(dj), csim._dp(w), csim._dp(r), 2.0, 0, 0]
    assert L.csim_obs_network_create_linear(None, *args, C.byref(out)) == 1 and not out.value
    assert L.csim_obs_network_create_linear(None, *args, None) == 1
    n = C.c_int(7)
    assert L.csim_obs_network_taps(None, C.byref(n)) == 1 and n.value == 7
